"""Widom insertion of foreign rigid solutes (mmc_batch_widom_solute / _at) against the oracle.

dU is defined as mmc_batch_widom's (include/mmc_hip.h): the change of potential(..., "ewald") when
the solute is appended as molecule N + 1, and the oracle is asked exactly that on a System of N + 1
molecules whose last one has the solute's S sites and its own atom types (solute_ref.SoluteOracle).
Tolerance: common.widom_close (1e-9 K + 1e-13 of the term) with the absolute part scaled by S / 3
for S > 3.

Shapes: R = 8 replicas x M = 32 insertions = 256 units on WV_WAVES = 4 waves per workgroup: with
"wave_wgs" = 1 each wave takes 64 insertions, with 2 each takes 32, by default every wave takes one.
NIST config 4 (750 SPC/E, r_cut 10) for the synthetic solutes, the 216-water TIP3P deck lattice
(r_cut 9) for MEA; both 300 device-proposed steps along their chains.  In the deck lattice (box
18.69 A) kappa = alpha / L with alpha = 5.5, not 5.6: the batch's erfc table, which the unit kernels
need, covers kappa sqrt(r_cut^2 + 100) <= 4, and 5.6 / 18.69 x sqrt(181) = 4.03."""
import ctypes

import numpy as np
import pytest

import common
import solute_ref as sr
from metropolismontecarlo_amd import _lib
from metropolismontecarlo_amd import observables as obs
from metropolismontecarlo_amd import structs

pytestmark = pytest.mark.gpu

RCUT = 10.0
T = sr.T


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def make_batch(a, R, rcut=RCUT, alpha=5.6):
    from metropolismontecarlo_amd.device import Batch
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
              alpha / a["box"], structs.factor, rcut, rcut)
    b.recip_long()
    return b


@pytest.fixture(scope="module")
def cfg4():
    return common.nist_arrays(4, "unwrapped")


@pytest.fixture(scope="module")
def diversified(cfg4):
    """NIST config 4, 8 replicas, each taken 300 device-proposed steps along its own chain."""
    b = make_batch(cfg4, 8)
    b.set_option("device_moves", 1)
    b.run(300, T, 0.3, 0.2, seed=4242)
    yield b
    b.close()


@pytest.fixture(scope="module")
def tip3p():
    return sr.tip3p_lattice()


@pytest.fixture(scope="module")
def tip3p_diversified(tip3p):
    b = make_batch(tip3p, 8, rcut=sr.MEA_RCUT, alpha=sr.MEA_ALPHA)
    b.set_option("device_moves", 1)
    b.run(300, T, 0.3, 0.2, seed=4243)
    yield b
    b.close()


def check_all(orc, a, b, sol, mol, du, ovl, rcut=RCUT, alpha=5.6):
    so = sr.SoluteOracle(orc, a, sol, rcut, rcut, alpha)
    out = [sr.check_solute(so, b, r, mol[r], du[r], ovl[r]) for r in range(b.R)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def test_water_as_a_foreign_solute(orc, cfg4, diversified):
    b = diversified
    sol = sr.water_solute(cfg4, b.widom_offsets)
    _, _, wmol, wdu, wovl = b.widom(32, T, seed=77, draw0=5, outputs=True)
    bs, no, mol, du, ovl = b.widom_solute(sol, 32, T, seed=77, draw0=5, outputs=True)
    assert mol.shape == (b.R, 32, 4, 3)
    assert mol.tobytes() == wmol.tobytes()
    assert np.array_equal(ovl, wovl)
    check_all(orc, cfg4, b, sol, mol, du, ovl)
    # ... and hence within twice the tolerance of widom's own terms
    assert np.all(np.abs(du - wdu) <= 2 * (1e-9 + 1e-13 * np.abs(wdu))), np.abs(du - wdu).max()
    assert np.all(np.isfinite(bs)) and np.array_equal(no, (ovl != 0).sum(1))


def test_neutral_one_site_solute(orc, cfg4, diversified):
    b = diversified
    sol = sr.methane(cfg4)
    bs, no, mol, du, ovl = b.widom_solute(sol, 32, T, seed=78, draw0=0, outputs=True)
    z = np.zeros_like(du[:, :, 1:])
    assert du[:, :, 1:].tobytes() == z.tobytes()          # exactly +0.0, sign included
    assert not ovl.any() and not no.any()
    assert mol[:, :, 0].tobytes() == mol[:, :, 1].tobytes()
    ref, _ = check_all(orc, cfg4, b, sol, mol, du, ovl)
    assert np.abs(ref[:, :, 0]).max() > 1.0               # the LJ term is not trivially zero
    # the reference points are widom's COMs of the same draws
    _, _, wmol, _, _ = b.widom(32, T, seed=78, draw0=0, outputs=True)
    assert mol[:, :, 1].tobytes() == np.ascontiguousarray(wmol[:, :, 9:]).tobytes()


@pytest.mark.parametrize("which", ["cation", "dipole"])
def test_charged_solutes(orc, cfg4, diversified, which):
    b = diversified
    sol = getattr(sr, which)(cfg4)
    bs, no, mol, du, ovl = b.widom_solute(sol, 32, T, seed=79, draw0=3, outputs=True)
    ref, flags = check_all(orc, cfg4, b, sol, mol, du, ovl)
    # the self term is part of d_recip (SoluteOracle adds orc.ewald_self of the solute's charges)
    self_d = -structs.factor * (5.6 / cfg4["box"]) / np.sqrt(np.pi) * (sol.charge ** 2).sum()
    assert abs(self_d) > 1e3
    assert np.all(du[:, :, 1][ovl == 1] == 0.0)
    assert np.array_equal(no, (ovl != 0).sum(1))


def test_mea_in_the_deck_lattice(orc, tip3p, tip3p_diversified):
    b = tip3p_diversified
    sol = sr.mea()
    bs, no, mol, du, ovl = b.widom_solute(sol, 32, T, seed=sr.MEA_SEED, draw0=sr.MEA_DRAW0, outputs=True)
    assert mol.shape == (b.R, 32, 12, 3)
    from metropolismontecarlo_amd.device import philox4x32
    for r in (0, 7):
        ref = obs.solute_molecules(philox4x32, sr.MEA_SEED, sr.MEA_DRAW0, 32, r, b.box, sol.offsets)
        assert np.abs(mol[r] - ref).max() <= 1e-12
    check_all(orc, tip3p, b, sol, mol, du, ovl, rcut=sr.MEA_RCUT, alpha=sr.MEA_ALPHA)
    share = np.count_nonzero(ovl & 1) / ovl.size
    print(f"MEA insertions flagged as overlaps: {np.count_nonzero(ovl & 1)} of {ovl.size}")
    assert 0.25 <= share <= 0.75, share


def test_sixteen_sites(orc, cfg4, diversified):
    b = diversified
    sol = sr.synthetic(cfg4, 16, seed=16)
    bs, no, mol, du, ovl = b.widom_solute(sol, 32, T, seed=80, draw0=1, outputs=True)
    assert mol.shape == (b.R, 32, 17, 3)
    ref, flags = check_all(orc, cfg4, b, sol, mol, du, ovl)
    assert flags.any() and not flags.all()


def test_edges_through_widom_solute_at(orc, cfg4):
    a = cfg4
    b = make_batch(a, 1)
    L = float(a["box"])
    com, coords, _ = b.get_replica(0)
    sol = sr.synthetic(a, 5, seed=5, extent=1.6)
    off, S = sol.offsets, sol.n_sites

    def upright(c):
        return np.vstack([np.asarray(c) + off, c])

    far = int(np.argmax(np.linalg.norm(off, axis=1)))       # the site farthest from the reference point
    mols = []
    # sites straddling the faces of the box
    mols.append(upright(np.array([0.2, L - 0.3, 15.0])))
    mols.append(upright(np.array([L - 0.1, 0.05, L - 0.2])))
    # the reference point at 0 and at L
    mols.append(upright(np.array([0.0, 0.0, 0.0])))
    mols.append(upright(np.array([L, L, L])))
    mols.append(upright(np.array([L, 7.0, 0.0])))
    # the reference point inside the gate of water j while the farthest site lies beyond r_cut of
    # its COM (and the other way round: the point outside, the site inside)
    u = off[far] / np.linalg.norm(off[far])
    for j in (3, 411):
        for f in (1 - 1e-12, 1 + 1e-12, 0.99):
            mols.append(upright((com[j] + RCUT * f * u) % L))
            mols.append(upright((com[j] - RCUT * f * u) % L))
    n_plain = len(mols)
    # a site on a water hydrogen with the opposite charge: an overlap, d_real = 0
    neg = int(np.argmin(sol.charge))
    assert sol.charge[neg] < 0 < a["charge"][1]
    mols.append(upright(coords[3 * 100 + 1] - off[neg]))
    mols = np.array(mols)[None]
    assert np.any(mols < 0) and np.any(mols > L)            # sites do leave the box
    bs, no, du, ovl = b.widom_solute_at(sol, mols, T)
    so = sr.SoluteOracle(orc, a, sol, RCUT, RCUT)
    ref, flags = sr.check_solute(so, b, 0, mols[0], du[0], ovl[0])
    assert ovl[0, n_plain] == 1 and du[0, n_plain, 1] == 0.0 and flags[n_plain]
    assert np.all(np.isfinite(du))
    hb, hn = common.widom_host_sums(du, ovl, [0.0], [0], T)
    assert no[0] == hn[0] and abs(bs[0] - hb[0]) <= 1e-14 * hb[0]
    # the same molecules through the generator's layout: _at of what widom_solute drew is widom_solute
    _, _, mol2, du2, ovl2 = b.widom_solute(sol, 8, T, seed=3, outputs=True)
    _, _, du3, ovl3 = b.widom_solute_at(sol, mol2, T)
    assert du2.tobytes() == du3.tobytes() and ovl2.tobytes() == ovl3.tobytes()
    with pytest.raises(ValueError):
        b.widom_solute_at(sol, np.zeros((1, 2, S, 3)), T)
    b.close()


def test_neighbour_list_flush(orc):
    """2000 SPC/E molecules compressed to 0.06 / A^3 (32.2 A) with a 12.4 A cutoff, the system of
    test_gpu_widom_paths.py's flush test: 430-520 COMs inside the gate of any point, more than the
    neighbour list holds, so every scan of k_solute_wave empties its list after a trip and goes on
    (asserted on the host, solute_ref.scan_flushes): a lane's sums add across process() calls.  A
    charged five-site solute and methane at the centres of the lattice's cells."""
    from test_gpu_batch import _dense_water
    a = _dense_water(2000, rho=0.06)
    L, rc = float(a["box"]), 12.4
    assert rc < L / 2 and rc * rc + 100 < 256 and 5.6 / L * np.sqrt(rc * rc + 100) < 4
    nc = int(round(np.cbrt(2197)))
    sp = L / nc
    rng = np.random.default_rng(2000)
    cells = rng.choice(nc ** 3, size=12, replace=False)
    b = make_batch(a, 1, rcut=rc)
    for sol in (sr.synthetic(a, 5, seed=5, extent=1.6), sr.methane(a)):
        mols = []
        for c in cells:
            i, j, k = c // (nc * nc), (c // nc) % nc, c % nc
            centre = (np.array([i, j, k]) + 0.51) * sp
            assert sr.scan_flushes(a["com"], centre, rc, L), c
            q = rng.normal(size=4)
            w, x, y, z = q / np.linalg.norm(q)
            rot = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
            mols.append(np.vstack([centre + sol.offsets @ rot.T, centre]))
        mols = np.array(mols)[None]
        bs, no, du, ovl = b.widom_solute_at(sol, mols, T)
        so = sr.SoluteOracle(orc, a, sol, rc, rc)
        ref, _ = sr.check_solute(so, b, 0, mols[0], du[0], ovl[0])
        assert np.abs(ref[:, 0]).max() > 1.0
    b.close()


def test_reductions_and_launch_shape(diversified, cfg4):
    b = diversified
    sol = sr.synthetic(cfg4, 7, seed=7)
    rng = np.random.default_rng(3)
    b0 = rng.random(b.R) * 1e-3
    n0 = rng.integers(0, 5, size=b.R).astype(np.int64)
    for s, M in ((sol, 32), (sr.methane(cfg4), 32), (sol, 1), (sol, 65)):
        runs = []
        for wgs in (0, 1, 2, 0):
            b.set_option("wave_wgs", wgs)
            runs.append(b.widom_solute(s, M, T, seed=91, draw0=0, boltz_sum=b0.copy(), n_overlap=n0.copy(),
                                       outputs=True))
        b.set_option("wave_wgs", 0)
        bs, no, _, du, ovl = runs[0]
        assert du.shape == (b.R, M, 3)
        # the in-order sums on the host; the weights' exp differs from numpy's by an ulp at most
        hb, hn = common.widom_host_sums(du, ovl, b0, n0, T)
        assert np.array_equal(no, hn)
        assert np.all(np.abs(bs - hb) <= 1e-14 * np.abs(hb)), (bs, hb)
        for other in runs[1:]:
            for x, y in zip(runs[0], other):
                assert x.tobytes() == y.tobytes()
    # a longer call is its shorter calls in a row: insertion j depends on (seed, draw0 + j) alone
    _, _, m65, d65, o65 = runs[0]
    _, _, m1, d1, o1 = b.widom_solute(sol, 1, T, seed=91, draw0=64, outputs=True)
    assert m65[:, 64:].tobytes() == m1.tobytes() and d65[:, 64:].tobytes() == d1.tobytes()
    assert o65[:, 64:].tobytes() == o1.tobytes()


def test_the_call_is_read_only(cfg4):
    R = 4
    sol = sr.synthetic(cfg4, 6, seed=6)
    twins = [make_batch(cfg4, R), make_batch(cfg4, R)]
    chains = []
    for b in twins:
        b.set_option("device_moves", 1)
        e = b.potential_ewald(as_array=True)["energy"]
        chains.append(b.new_chains(e))
    b = twins[0]
    before = [b.get_replica(r) for r in range(R)]
    b.widom_solute(sol, 16, T, seed=5)
    b.widom_solute(sr.methane(cfg4), 16, T, seed=5)
    after = [b.get_replica(r) for r in range(R)]
    for x, y in zip(before, after):
        for u, v in zip(x, y):
            assert u.tobytes() == v.tobytes()
    acc = (np.zeros(R), np.zeros(R, dtype=np.int64))
    for blk in range(3):
        for b, c in zip(twins, chains):
            b.run_chains(c, 200, T, seed=808)
        twins[0].widom_solute(sol, 8, T, seed=9, draw0=8 * blk, boltz_sum=acc[0], n_overlap=acc[1])
    assert chains[0].tobytes() == chains[1].tobytes()
    for r in range(R):
        for u, v in zip(twins[0].get_replica(r), twins[1].get_replica(r)):
            assert u.tobytes() == v.tobytes()
    # (a replica whose 24 insertions all overlap or land on a repulsive core has a sum of 0)
    assert np.all(np.isfinite(acc[0])) and np.all(acc[0] >= 0) and acc[0].sum() > 0
    assert np.all((acc[1] >= 0) & (acc[1] <= 24))
    for b in twins:
        b.close()


def test_scope_and_refusals_leave_outputs_untouched(cfg4):
    a = cfg4
    R = 2
    sol = sr.dipole(a)

    def expect(b, status):
        for at in (False, True):
            bs, no = np.full(R, 7.5), np.full(R, 3, dtype=np.int64)
            with pytest.raises(_lib.MMCError) as ei:
                if at:
                    b.widom_solute_at(sol, np.zeros((R, 2, 3, 3)) + 5.0, T, boltz_sum=bs, n_overlap=no)
                else:
                    b.widom_solute(sol, 4, T, 1, boltz_sum=bs, n_overlap=no)
            assert ei.value.status == status, (at, ei.value)
            assert np.all(bs == 7.5) and np.all(no == 3)

    # per-replica boxes
    b = make_batch(a, R)
    b.set_boxes([a["box"], a["box"] * 1.01], 5.6)
    expect(b, _lib.MMC_ERR_UNSUPPORTED)
    b.close()
    # Wolf style
    b = make_batch(a, R)
    b.set_coulomb_style("wolf")
    expect(b, _lib.MMC_ERR_UNSUPPORTED)
    b.close()
    # proposals outstanding
    b = make_batch(a, R)
    com, coords = np.asarray(a["com"]), np.asarray(a["coords"])
    b.eval(np.full(R, 3), np.tile(com[2], (R, 1)), np.tile(coords[6:9], (R, 1, 1)))
    expect(b, _lib.MMC_ERR_STATE)
    b.settle(np.zeros(R, dtype=np.int32))
    # with a batch: the raw outputs of the C call stay untouched too, and non-finite molecules are refused
    L = _lib.lib()
    dp = lambda x: x.ctypes.data_as(_lib._dp)  # noqa: E731
    bs, no = np.full(R, 7.5), np.full(R, 3, dtype=np.int64)
    mol = np.full((R, 2, 3, 3), 5.0)
    mol[1, 1, 2, 0] = np.nan
    du, ov = np.full((R, 2, 3), 7.5), np.full((R, 2), 9, dtype=np.uint8)
    st = L.mmc_batch_widom_solute_at(b._h, 2, dp(sol.charge), dp(sol.eps), dp(sol.sig), 2, dp(mol), T, dp(bs),
                                     no.ctypes.data_as(_lib._i64p), dp(du),
                                     ov.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    assert st == _lib.MMC_ERR_ARG
    assert np.all(bs == 7.5) and np.all(no == 3) and np.all(du == 7.5) and np.all(ov == 9)
    # ... and after all that the call works
    bs, no = b.widom_solute(sol, 4, T, 1)
    assert np.all(bs > 0)
    b.close()
