"""Host side of Widom insertion (no GPU): the generator's host mirror (Shoemake rotations, COMs in
[0, L)), the orientation distribution's moments, and the two observables' arithmetic."""
import math

import numpy as np

from metropolismontecarlo_amd import observables as obs


def _philox_py(ctr, key):
    """Philox4x32-10 in plain Python (csrc/mmc_propose.hpp), independent of the library."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    M = 0xffffffff
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M, p1 & M, ((p0 >> 32) ^ c3 ^ k1) & M, p0 & M
        k0, k1 = (k0 + 0x9E3779B9) & M, (k1 + 0xBB67AE85) & M
    return [c0, c1, c2, c3]


def test_philox_known_answer():
    # Salmon et al.'s known-answer vector for Philox4x32-10 (counter 0, key 0)
    assert _philox_py([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]


OFF = np.array([[0.0, 0.0, -0.0646], [0.8165, 0.0, 0.5127], [-0.8165, 0.0, 0.5127]])


def test_mirror_rotations_are_proper_and_coms_inside_the_box():
    box = 30.0
    mol = obs.widom_molecules(_philox_py, 0xdeadbeefcafe, 17, 200, 5, box, OFF)
    com = mol[:, 9:]
    assert np.all((com >= 0.0) & (com < box))
    for j in range(mol.shape[0]):
        at = mol[j, :9].reshape(3, 3) - com[j]
        # R maps the offsets onto the atoms: solve and check R^T R = 1, det R = +1
        u1, u2, u3 = (obs.philox_uniforms(_philox_py, 0xdeadbeefcafe, 17 + j, obs.MMC_SLOT_WIDOM + 1, 5)[1],
                      *obs.philox_uniforms(_philox_py, 0xdeadbeefcafe, 17 + j, obs.MMC_SLOT_WIDOM + 2, 5))
        R = obs.shoemake_rotation(u1, u2, u3)
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-14
        assert abs(np.linalg.det(R) - 1.0) < 1e-14
        assert np.abs(at - OFF @ R.T).max() < 1e-14


def test_orientation_distribution_is_uniform():
    """10^5 rotations of the generator's map from uniforms: the moments of the Haar measure on
    SO(3) -- <R_ij> = 0, <R_ij^2> = 1/3, <tr R> = 0, <(tr R)^2> = 1 -- and the rotation angle's
    density (1 - cos t) / pi, whose <cos t> = -1/2."""
    rng = np.random.default_rng(5)
    n = 100_000
    u = rng.random((n, 3))
    s1, s2 = np.sqrt(1.0 - u[:, 0]), np.sqrt(u[:, 0])
    a, b = 2 * np.pi * u[:, 1], 2 * np.pi * u[:, 2]
    w, x, y, z = s2 * np.cos(b), s1 * np.sin(a), s1 * np.cos(a), s2 * np.sin(b)
    Rs = np.empty((n, 3, 3))
    Rs[:, 0, 0] = 1 - 2 * (y * y + z * z); Rs[:, 0, 1] = 2 * (x * y - w * z); Rs[:, 0, 2] = 2 * (x * z + w * y)
    Rs[:, 1, 0] = 2 * (x * y + w * z); Rs[:, 1, 1] = 1 - 2 * (x * x + z * z); Rs[:, 1, 2] = 2 * (y * z - w * x)
    Rs[:, 2, 0] = 2 * (x * z - w * y); Rs[:, 2, 1] = 2 * (y * z + w * x); Rs[:, 2, 2] = 1 - 2 * (x * x + y * y)
    # the vectorised form is the mirror's function
    for k in (0, 1, 777):
        assert np.abs(Rs[k] - obs.shoemake_rotation(*u[k])).max() < 1e-15
    se = 4.0 / math.sqrt(n)  # ~4 standard errors of a mean of a variable of variance <= 1
    assert np.abs(Rs.mean(0)).max() < se
    assert np.abs((Rs ** 2).mean(0) - 1.0 / 3.0).max() < se
    tr = np.trace(Rs, axis1=1, axis2=2)
    assert abs(tr.mean()) < 2 * se and abs((tr ** 2).mean() - 1.0) < 4 * se
    # the rotation angle: density (1 - cos t) / pi on [0, pi], so <cos t> = -1/2
    cos_t = (tr - 1.0) / 2.0
    assert abs(cos_t.mean() + 0.5) < se


def test_widom_mu_ex_by_hand():
    T = 300.0
    assert obs.widom_mu_ex(10.0, 10, T) == 0.0
    assert abs(obs.widom_mu_ex(5.0, 10, T) - (-T * math.log(0.5))) < 1e-12
    w = [math.exp(-(-1200.0) / T), math.exp(-(300.0) / T), 0.0]
    assert abs(obs.widom_mu_ex(sum(w), 3, T) - (-T * math.log(sum(w) / 3))) < 1e-9
    v = obs.widom_mu_ex(np.array([1.0, 4.0]), 2, T)
    assert np.allclose(v, [-T * math.log(0.5), -T * math.log(2.0)], rtol=0, atol=1e-12)


def test_ewald_intra_energy_by_hand():
    q = [-0.8476, 0.4238, 0.4238]
    kappa, factor = 5.6 / 30.0, 167101.0
    r_oh, r_hh = np.linalg.norm(OFF[0] - OFF[1]), np.linalg.norm(OFF[1] - OFF[2])
    want = factor * (2 * q[0] * q[1] * math.erf(kappa * r_oh) / r_oh + q[1] * q[2] * math.erf(kappa * r_hh) / r_hh)
    assert abs(obs.ewald_intra_energy(OFF, q, kappa, factor) - want) < 1e-9 * abs(want)
    # two unit charges 2 A apart
    assert abs(obs.ewald_intra_energy([[0, 0, 0], [0, 0, 2.0]], [1.0, -1.0], 0.5, 1.0)
               - (-math.erf(1.0) / 2.0)) < 1e-15


def test_scan_flush_helper_on_a_hand_built_line():
    """common.scan_flushes, which the GPU tests use to show that a scan of mmc_wave_unit.inc empties
    its neighbour list mid-scan, on molecules laid out by hand: gated ones 0.01 A apart around the
    centre, the others 40 A away, in a 1000 A box."""
    import common
    n_list, n_pf = common._wave_list_consts()
    trip, thr = 64 * n_pf, n_list - 64 * n_pf
    assert (trip, thr) == (384, 256)
    box, gate, centre = 1000.0, 10.0, np.array([5.0, 500.0, 500.0])

    def line(gated):
        com = np.tile(centre + np.array([0.0, 40.0, 0.0]), (len(gated), 1))
        for j, g in enumerate(gated):
            if g:
                com[j] = centre + np.array([0.01 * (j % 500) - 2.5, 0.0, 0.0])
        return com

    def case(n_before, after_at, n=900, j_begin=0, exclude=None):
        g = np.zeros(n, dtype=bool)
        g[j_begin:j_begin + n_before] = True
        if after_at is not None:
            g[after_at] = True
        return common.scan_flushes(line(g), [centre], gate, box, j_begin=j_begin, exclude=exclude)

    assert case(257, 384)                 # 257 before the first trip boundary, one at it
    assert case(257, 899)
    assert not case(256, 384)             # not more than the threshold
    assert not case(300, None)            # nothing left after the boundary
    assert not case(257, 384, exclude=3)  # the unit's own molecule does not count
    assert not case(257, 383, n=384)      # no boundary inside [0, n): the scan ends in one trip
    # boundaries follow j_begin: [100, 484) is the first trip
    assert case(257, 484, j_begin=100)
    assert not case(257, 483, j_begin=100)
    # two centres (a move's old and new COM) gate their union; the minimum image counts
    g = np.zeros(900, dtype=bool)
    g[:200] = True
    g[400] = True
    com = line(g)
    com[200:260] = centre + np.array([-12.0, 0.0, 0.0])         # gated by the second centre only
    assert not common.scan_flushes(com, [centre], gate, box)
    assert common.scan_flushes(com, [centre, centre + np.array([-8.0, 0.0, 0.0])], gate, box)
    com[200:260] = centre + np.array([-12.0 + box, 0.0, 0.0])    # the same through the boundary
    assert common.scan_flushes(com, [centre, centre + np.array([-8.0, 0.0, 0.0])], gate, box)
    # the exact gate, by a margin: a COM on the gate does not count
    com[:200] = centre + np.array([0.0, gate, 0.0])
    assert not common.scan_flushes(com, [centre, centre + np.array([-8.0, 0.0, 0.0])], gate, box)
