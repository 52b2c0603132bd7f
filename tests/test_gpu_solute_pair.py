"""Widom insertion of solute pairs (mmc_batch_widom_pair / _at) against the oracle.

Per insertion and separation the library returns three rows of (lj, real, recip): dA and dB_k are
mmc_batch_widom_solute's terms, checked with solute_ref.SoluteOracle on N + 1 molecules; x_k is the
A-B interaction, checked with the oracle's lj_poly_du(2), ewald_short(2) and factor (recip_long(A u B)
- recip_long(A) - recip_long(B)) on a System that holds only A and B (solute_pair_ref.PairOracle).
Tolerance: solute_ref.solute_close with S = S_A for A, S_B for B and S_A + S_B for x.

Shapes: R = 8 replicas x M = 8 insertions x K = 4 separations on NIST config 4 (750 SPC/E, r_cut 10),
300 device-proposed steps along each chain: 64 units on WV_WAVES = 4 waves per workgroup, five
placements per unit = two tiles of k_solute_pair_wave's pair part."""
import numpy as np
import pytest

import common
import solute_pair_ref as pr
import solute_ref as sr
from metropolismontecarlo_amd import _lib
from metropolismontecarlo_amd import structs

pytestmark = pytest.mark.gpu

RCUT, T, M = pr.RCUT, pr.T, pr.M
SUMS = ("boltz_a", "n_zero_a", "boltz_b", "n_zero_b", "boltz_ab", "n_zero_ab")


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
    b = make_batch(cfg4, pr.R)
    b.set_option("device_moves", 1)
    b.run(300, T, 0.3, 0.2, seed=4242)
    yield b
    b.close()


def check_all(orc, a, b, pair, mol_a, mol_b, du, fl, rcut=RCUT):
    po = pr.PairOracle(orc, a, pair, rcut, rcut)
    out = [pr.check_pair(po, b, r, mol_a[r], mol_b[r], du[r], fl[r]) for r in range(b.R)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def same(x, y):
    return x.tobytes() == y.tobytes()


def test_methane_methane(orc, cfg4, diversified):
    b = diversified
    pair = pr.methane_pair(cfg4)
    d = (3.9, 5.5, 7.0, 11.0)
    sm, ma, mb, du, fl = b.widom_pair(pair, d, M, T, seed=81, draw0=4, outputs=True)
    assert ma.shape == (b.R, M, 2, 3) and mb.shape == (b.R, M, 4, 2, 3)
    assert du.shape == (b.R, M, 9, 3) and fl.shape == (b.R, M, 5)
    assert same(du[..., 1:], np.zeros_like(du[..., 1:]))        # exactly +0.0, sign included
    x_lj = du[:, :, 5:, 0]
    assert np.all(x_lj[:, :, 3] == 0.0) and np.all(x_lj[:, :, 0] != 0.0)   # the gate is closed at 11 A
    ref, _ = check_all(orc, cfg4, b, pair, ma, mb, du, fl)
    assert np.abs(ref[:, :, :5, 0]).max() > 1.0
    assert not fl.any() and not any(sm[k].any() for k in SUMS[1::2])
    # A is widom_solute's solute of the same draws, and its terms within twice the tolerance
    _, _, smol, sdu, _ = b.widom_solute(pair.a, M, T, seed=81, draw0=4, outputs=True)
    assert same(ma, smol)
    assert np.all(np.abs(du[:, :, 0] - sdu) <= 2 * (1e-9 + 1e-13 * np.abs(sdu)))
    # the separations are those asked for
    sep = mb[:, :, :, 1] - ma[:, :, None, 1]
    sep = sep + common.image_shift(sep, b.box)
    assert np.abs(np.linalg.norm(sep, axis=3) - np.array(d)).max() <= 1e-12


def test_cation_anion(orc, cfg4, diversified):
    b = diversified
    pair = pr.ion_pair(cfg4)
    sm, ma, mb, du, fl = b.widom_pair(pair, (0.5, 2.8, 6.0, 11.0), M, T, seed=82, draw0=1, outputs=True)
    check_all(orc, cfg4, b, pair, ma, mb, du, fl)
    x = du[:, :, 5:]
    # 0.5 A apart: r^2 = 0.25 < 0.5 with opposite charges, an A-B overlap on every insertion
    assert np.all(fl[:, :, 1] & 4) and np.all(x[:, :, 0, 1] == 0.0)
    assert np.array_equal(sm["n_zero_ab"][:, 0], np.full(b.R, M)) and np.all(sm["boltz_ab"][:, 0] == 0.0)
    assert not np.any(fl[:, :, 2:] & 4)
    # 11 A apart: beyond both gates, the reciprocal term remains
    assert np.all(x[:, :, 3, 0] == 0.0) and np.all(x[:, :, 3, 1] == 0.0) and np.all(x[:, :, 3, 2] != 0.0)
    assert np.all(x[:, :, 1, 1] < -1e4)                        # the contact pair's attraction


@pytest.mark.parametrize("which", ["synthetic", "water_dipole"])
def test_multi_site_pairs(orc, cfg4, diversified, which):
    b = diversified
    pair = pr.synthetic_pair(cfg4) if which == "synthetic" else pr.water_dipole_pair(cfg4, b.widom_offsets)
    sm, ma, mb, du, fl = b.widom_pair(pair, pr.MULTI_D, M, T, seed=pr.MULTI_SEED, draw0=pr.MULTI_DRAW0, outputs=True)
    assert ma.shape == (b.R, M, pair.a.n_sites + 1, 3) and mb.shape == (b.R, M, 4, pair.b.n_sites + 1, 3)
    ref, rfl = check_all(orc, cfg4, b, pair, ma, mb, du, fl)
    if which == "synthetic":
        assert (rfl != 0).any() and not (rfl != 0).all()
        assert (fl != 0).any() and not (fl != 0).all()
    # the counts are the flagged insertions
    assert np.array_equal(sm["n_zero_a"], (fl[:, :, 0] != 0).sum(1))
    assert np.array_equal(sm["n_zero_b"], ((fl[:, :, 1:] & 3) != 0).sum(1))
    assert np.array_equal(sm["n_zero_ab"], ((fl[:, :, 1:] | fl[:, :, :1]) != 0).sum(1))


def test_whole_potential_difference(orc, cfg4, diversified):
    """The oracle's potential(N + 2) - potential(N) against the device's dU_AB = (dU_A + dU_B) + x on
    replica 0, for the insertions without flags.  The margin covers the cancellation in a difference
    of two totals: test_solute_pair_host.py measures |oracle's sum of terms - oracle's difference of
    totals| for these draws at 1.01e-15 of the larger total (dU_AB runs up to 1e14 K for a solute on
    a repulsive core, so the measure is relative to the totals); allowed is four times
    pr.WHOLE_CANCELLATION = 1.1e-15 of the larger total plus the tolerances of the nine terms."""
    from test_solute_pair_host import WHOLE_D, WHOLE_DRAW0, WHOLE_SEED
    b = diversified
    com, coords, _ = b.get_replica(0)
    n = 0
    for pair in (pr.water_dipole_pair(cfg4, b.widom_offsets), pr.methane_pair(cfg4)):
        po = pr.PairOracle(orc, cfg4, pair)
        SA, SB = pair.a.n_sites, pair.b.n_sites
        sm, ma, mb, du, fl = b.widom_pair(pair, WHOLE_D, M, T, seed=WHOLE_SEED, draw0=WHOLE_DRAW0, outputs=True)
        _, _, _, du_ab = pr.du_total(du[0])
        for j in range(M):
            for k in range(len(WHOLE_D)):
                if fl[0, j, 0] or fl[0, j, 1 + k]:
                    continue
                diff, scale = po.total_difference(com, coords, ma[0, j], mb[0, j, k], b.box, key=id(b))
                rows = du[0, j, [0, 1 + k, 1 + len(WHOLE_D) + k]]
                tol = sum(1e-9 * max(1.0, S / 3.0) * 3 + 1e-13 * np.abs(row).sum()
                          for S, row in zip((SA, SB, SA + SB), rows))
                err = abs(du_ab[j, k] - diff)
                print(pair, j, k, du_ab[j, k], err, 4 * pr.WHOLE_CANCELLATION * scale + tol)
                assert err <= 4 * pr.WHOLE_CANCELLATION * scale + tol, (pair, j, k, du_ab[j, k], diff)
                n += 1
    assert n >= 16, n


def test_identities(cfg4, diversified):
    b = diversified
    d = (3.0, 4.5, 6.5, 11.0)
    rng = np.random.default_rng(7)
    # a ghost B: dU_AB is dU_A, so boltz_ab is boltz_a bit for bit, and every B weighs 1
    A = sr.synthetic(cfg4, 6, seed=6)
    for a_sol in (A, sr.methane(cfg4)):
        pair = structs.SolutePair(a_sol, pr.ghost(2), np.zeros((a_sol.n_sites, 2)), np.zeros((a_sol.n_sites, 2)))
        s0 = b.pair_sums(None, 4)
        s0["boltz_a"][:] = rng.random(b.R) * 1e-3
        s0["boltz_ab"][:] = s0["boltz_a"][:, None]
        s0["boltz_b"][:] = rng.integers(0, 9, size=(b.R, 4))
        b0 = s0["boltz_b"].copy()
        sm, ma, mb, du, fl = b.widom_pair(pair, d, M, T, seed=84, sums=s0, outputs=True)
        for k in range(4):
            assert same(sm["boltz_ab"][:, k], sm["boltz_a"])
            assert np.array_equal(sm["n_zero_ab"][:, k], sm["n_zero_a"])
        assert np.array_equal(sm["boltz_b"], b0 + M) and not sm["n_zero_b"].any()
        assert np.all(du[:, :, 1:] == 0.0)
    # _at of what widom_pair drew is widom_pair
    pair = pr.synthetic_pair(cfg4, 4, 7)
    sm, ma, mb, du, fl = b.widom_pair(pair, d, M, T, seed=85, draw0=9, outputs=True)
    sm2, du2, fl2 = b.widom_pair_at(pair, ma, mb, T)
    assert same(du, du2) and same(fl, fl2)
    for k in SUMS:
        assert same(sm[k], sm2[k])
    # A and B swapped, placements swapped (one separation at a time): dA and dB change places, x stays
    sw = pair.swapped()
    SA, SB = pair.a.n_sites, pair.b.n_sites
    for k in range(4):
        _, du3, fl3 = b.widom_pair_at(sw, np.ascontiguousarray(mb[:, :, k]), np.ascontiguousarray(ma[:, :, None]), T)
        for row3, row, S in ((0, 1 + k, SB), (1, 0, SA), (2, 5 + k, SA + SB)):
            x, y = du3[:, :, row3], du[:, :, row]
            assert np.all(np.abs(x - y) <= 2 * (1e-9 * max(1.0, S / 3.0) + 1e-13 * np.abs(y))), (k, row)
        assert np.array_equal(fl3[:, :, 0] & 1, fl[:, :, 1 + k] & 1)
        assert np.array_equal(fl3[:, :, 1] & 5, (fl[:, :, 0] & 1) | (fl[:, :, 1 + k] & 4))
    with pytest.raises(ValueError):
        b.widom_pair_at(pair, ma, mb[:, :, :, :-1], T)


def test_edges_through_widom_pair_at(orc, cfg4):
    a = cfg4
    b = make_batch(a, 1)
    com, coords, _ = b.get_replica(0)
    pair = pr.edge_pair(a)
    mol_a, mol_b, names = pr.edge_cases(a, pair, com, coords)
    sm, du, fl = b.widom_pair_at(pair, mol_a, mol_b, T)
    po = pr.PairOracle(orc, a, pair)
    ref, rfl = pr.check_pair(po, b, 0, mol_a[0], mol_b[0], du[0], fl[0])
    j = names.index("overlap")
    assert fl[0, j, 1] & 1 and du[0, j, 1, 1] == 0.0 and not fl[0, j, 0] & 1
    assert sm["n_zero_ab"][0, 0] >= 1 and sm["n_zero_b"][0, 0] >= 1
    # on either side of the A-B gate
    g = [i for i, nm in enumerate(names) if nm.startswith("gate")]
    x = du[0][g][:, 3:]
    assert (x[:, :, 0] == 0.0).any() and (x[:, :, 0] != 0.0).any()
    assert np.array_equal(x[:, :, 0] == 0.0, x[:, :, 1] == 0.0) and np.all(x[:, :, 2] != 0.0)
    assert np.all(np.isfinite(du))
    hs = pr.host_sums(du, fl, b.pair_sums(None, 2), T)
    for k in SUMS[1::2]:
        assert np.array_equal(sm[k], hs[k]), k
    for k in SUMS[0::2]:
        assert np.all(np.abs(sm[k] - hs[k]) <= 1e-14 * np.abs(hs[k])), k
    b.close()


def test_neighbour_list_flush(orc):
    """The dense 2000-molecule system of test_gpu_solute.py's flush test (0.06 / A^3, r_cut 12.4):
    the union of a tile's gates holds more COMs than the neighbour list, so the scan of EVERY tile of
    every unit empties its list after a trip and goes on (asserted on the host from the kernel's own
    constants, solute_pair_ref.tile_scans_flush): a lane's sums of all the tile's placements add
    across process() calls.  Six placements per unit = two tiles."""
    a = pr.dense_water()
    L, rc = float(a["box"]), pr.FLUSH_RCUT
    b = make_batch(a, 1, rcut=rc)
    for pair in (pr.synthetic_pair(a, 3, 4), pr.methane_pair(a)):
        mol_a, mol_b = pr.flush_cases(a, pair)
        for j in range(mol_a.shape[1]):
            assert pr.tile_scans_flush(a["com"], mol_a[0, j, -1], mol_b[0, j, :, -1], rc, L), j
        sm, du, fl = b.widom_pair_at(pair, mol_a, mol_b, T)
        po = pr.PairOracle(orc, a, pair, rc, rc)
        ref, _ = pr.check_pair(po, b, 0, mol_a[0], mol_b[0], du[0], fl[0])
        assert np.abs(ref[:, :6, 0]).max() > 1.0
    b.close()


def test_reductions_and_launch_shape(diversified, cfg4):
    b = diversified
    pair = pr.synthetic_pair(cfg4, 4, 7)
    d = (2.5, 4.0, 6.0, 11.0)
    rng = np.random.default_rng(3)

    def start():
        s = b.pair_sums(None, 4)
        r = np.random.default_rng(11)
        for k in SUMS[0::2]:
            s[k][...] = r.random(s[k].shape) * 1e-3
        for k in SUMS[1::2]:
            s[k][...] = r.integers(0, 5, size=s[k].shape)
        return s

    for p, Mi in ((pair, 8), (pr.methane_pair(cfg4), 8), (pair, 1), (pair, 65)):
        runs = []
        for wgs in (0, 1, 2, 0):
            b.set_option("wave_wgs", wgs)
            runs.append(b.widom_pair(p, d, Mi, T, seed=91, draw0=0, sums=start(), outputs=True))
        b.set_option("wave_wgs", 0)
        sm, ma, mb, du, fl = runs[0]
        assert du.shape == (b.R, Mi, 9, 3)
        hs = pr.host_sums(du, fl, start(), T)
        for k in SUMS[1::2]:
            assert np.array_equal(sm[k], hs[k]), k
        for k in SUMS[0::2]:
            assert np.all(np.abs(sm[k] - hs[k]) <= 1e-14 * np.abs(hs[k])), (k, sm[k], hs[k])
        for other in runs[1:]:
            for k in SUMS:
                assert same(sm[k], other[0][k]), k
            for x, y in zip(runs[0][1:], other[1:]):
                assert same(x, y)
    # a longer call is its shorter calls in a row: insertion j depends on (seed, draw0 + j) alone
    _, a65, b65, d65, f65 = runs[0]
    _, a1, b1, d1, f1 = b.widom_pair(pair, d, 1, T, seed=91, draw0=64, outputs=True)
    assert same(a65[:, 64:], a1) and same(b65[:, 64:], b1) and same(d65[:, 64:], d1) and same(f65[:, 64:], f1)
    s_long = b.widom_pair(pair, d, 16, T, seed=92)
    s_two = b.widom_pair(pair, d, 8, T, seed=92)
    s_two = b.widom_pair(pair, d, 8, T, seed=92, draw0=8, sums=s_two)
    for k in SUMS:
        assert same(s_long[k], s_two[k]), k
    del rng


def test_the_call_is_read_only(cfg4):
    R = 4
    pair = pr.synthetic_pair(cfg4, 4, 7)
    d = (3.0, 6.0, 9.0)
    twins = [make_batch(cfg4, R), make_batch(cfg4, R)]
    chains = []
    for b in twins:
        b.set_option("device_moves", 1)
        e = b.potential_ewald(as_array=True)["energy"]
        chains.append(b.new_chains(e))
    b = twins[0]
    before = [b.get_replica(r) for r in range(R)]
    b.widom_pair(pair, d, 8, T, seed=5)
    b.widom_pair(pr.methane_pair(cfg4), d, 8, T, seed=5)
    after = [b.get_replica(r) for r in range(R)]
    for x, y in zip(before, after):
        for u, v in zip(x, y):
            assert same(u, v)
    acc = None
    for blk in range(3):
        for b, c in zip(twins, chains):
            b.run_chains(c, 200, T, seed=808)
        acc = twins[0].widom_pair(pair, d, 4, T, seed=9, draw0=4 * blk, sums=acc)
    assert chains[0].tobytes() == chains[1].tobytes()
    for r in range(R):
        for u, v in zip(twins[0].get_replica(r), twins[1].get_replica(r)):
            assert same(u, v)
    assert all(np.all(np.isfinite(acc[k])) and np.all(acc[k] >= 0) for k in SUMS[0::2])
    assert all(np.all((acc[k] >= 0) & (acc[k] <= 12)) for k in SUMS[1::2])
    for b in twins:
        b.close()


def test_scope_and_refusals_leave_outputs_untouched(cfg4):
    a = cfg4
    R = 2
    pair = pr.water_dipole_pair(a, pr.water_offsets(a))
    d = (3.0, 5.0)

    def sentinels(b):
        s = b.pair_sums(None, 2)
        for k in SUMS[0::2]:
            s[k][...] = 7.5
        for k in SUMS[1::2]:
            s[k][...] = 3
        return s

    def untouched(s):
        return all(np.all(s[k] == 7.5) for k in SUMS[0::2]) and all(np.all(s[k] == 3) for k in SUMS[1::2])

    def expect(b, status, d=d):
        for at in (False, True):
            s = sentinels(b)
            with pytest.raises(_lib.MMCError) as ei:
                if at:
                    b.widom_pair_at(pair, np.zeros((R, 2, 4, 3)) + 5.0, np.zeros((R, 2, 2, 3, 3)) + 6.0, T, sums=s)
                else:
                    b.widom_pair(pair, d, 4, T, 1, sums=s)
            assert ei.value.status == status, (at, ei.value)
            assert untouched(s)

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
    # a separation of half the box and more: refused with the batch, outputs untouched
    for bad in ((3.0, a["box"] / 2), (a["box"], 3.0)):
        s = sentinels(b)
        with pytest.raises(_lib.MMCError) as ei:
            b.widom_pair(pair, bad, 4, T, 1, sums=s)
        assert ei.value.status == _lib.MMC_ERR_ARG and "half the box" in str(ei.value) and untouched(s)
    # non-finite placements
    s = sentinels(b)
    mb = np.zeros((R, 2, 2, 3, 3)) + 6.0
    mb[1, 1, 1, 2, 0] = np.nan
    with pytest.raises(_lib.MMCError) as ei:
        b.widom_pair_at(pair, np.zeros((R, 2, 4, 3)) + 5.0, mb, T, sums=s)
    assert ei.value.status == _lib.MMC_ERR_ARG and "mol_b_in" in str(ei.value) and untouched(s)
    # ... and after all that the call works
    sm = b.widom_pair(pair, (3.0, b.box / 2 * (1 - 1e-12)), 4, T, 1)
    assert np.all(sm["boltz_b"] >= 0) and np.all(np.isfinite(sm["boltz_ab"]))
    b.close()
