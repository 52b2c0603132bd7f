"""mmc_batch_orient_corr against its numpy restatement (tests/orient_ref.py) on SPC/E molecules of
the NIST fixtures, truncated to the sizes at which k_orient_corr_wave takes another path.

Launch shape: the unit is k_rdf_sites_wave's 64 x 64 tile of the i < j triangle, K (K + 1) / 2 per
replica with K = ceil(N / 64); wave W of the launch's NW takes the contiguous run
[n_tiles W / NW, n_tiles (W + 1) / NW).  N = 70 and 129 are the smallest sizes with a partial last
block, a half-masked diagonal tile and an off-diagonal tile; with option wave_wgs = 1 four waves
share the 18 tiles of three replicas of 129 molecules, so a wave crosses replica boundaries and
flushes its counters in between.

Bounds.  Row 0 is exact.  Rows 1..3: the device may evaluate a pair's value within 2^-31 of the
restatement's (include/mmc_hip.h), two values that close round to integers at most 1 apart, and
each pair contributes once: per slot |device - restatement| <= row 0 of that slot, in units."""
import numpy as np
import pytest

import common
import orient_ref as oref
from metropolismontecarlo_amd import _lib, structs

pytestmark = pytest.mark.gpu

RCUT = 9.0                      # below L / 2 = 10 of the 20 A fixtures: r_max = r_cut differs from L / 2
RCUT_PB = 10.0                  # per-replica boxes: the erfc table covers kappa = alpha / (2 r_cut) from here
T, DR, DPHI = 298.15, 0.3, 0.2
ALPHA = 5.6
UNIT = 2 ** 30
SIZES = (1, 2, 63, 64, 70, 129)


def truncated(n_mol):
    """The first n_mol molecules of NIST configuration 1 (100 molecules) or 2 (200), L = 20 A."""
    a = common.nist_arrays(1 if n_mol <= 100 else 2, "unwrapped")
    return dict(a, com=a["com"][:n_mol], coords=a["coords"][:3 * n_mol], atype=a["atype"][:3 * n_mol],
                charge=a["charge"][:3 * n_mol])


def make_batch(a, R, rcut=RCUT):
    from metropolismontecarlo_amd.device import Batch
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
              ALPHA / a["box"], structs.factor, rcut, rcut)
    b.recip_long()
    return b


def diversify(b, a, seed):
    """Every replica but the first gets its own configuration: each molecule turned rigidly about
    its centre of mass by a random rotation and shifted by up to 0.4 A."""
    rng = np.random.default_rng(seed)
    n = a["com"].shape[0]
    for r in range(1, b.R):
        q = rng.normal(size=(n, 4))
        q /= np.linalg.norm(q, axis=1)[:, None]
        w, x, y, z = q.T
        rot = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                        [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                        [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]).transpose(2, 0, 1)
        off = a["coords"].reshape(n, 3, 3) - a["com"][:, None, :]
        com = a["com"] + (rng.random((n, 3)) - 0.5) * 0.8
        coords = com[:, None, :] + np.einsum("nij,naj->nai", rot, off)
        b.set_replica(r, com, coords.reshape(-1, 3))


def want_rows(b, charge, boxes, numbins, r_max, reverse=False):
    """[R, 4, numbins + 2] from the batch's own coordinates, each replica at its box."""
    out = []
    for r in range(b.R):
        com, coords, _ = b.get_replica(r)
        out.append(oref.orient_rows(com, coords, charge, float(boxes[r]), numbins, r_max, reverse=reverse))
    return np.stack(out)


def check_against(per, tot, want, n_mol, what):
    R, numbins = want.shape[0], want.shape[2] - 2
    assert per.dtype == np.int64 and per.shape == want.shape and tot.shape == want.shape[1:], what
    assert np.array_equal(per[:, 0], want[:, 0]), (what, "row 0")
    assert np.all(per[:, 0].sum(-1) == n_mol * (n_mol - 1) // 2), what
    assert np.all(per[:, 0, -1] == n_mol * (n_mol - 1) // 2 - per[:, 0, :-1].sum(-1)), what
    assert np.all(per[:, 2:, -1] == 0), (what, "rows 2 and 3 beyond r_max")
    for row in (1, 2, 3):
        err = np.abs(per[:, row] - want[:, row])
        print(f"{what} row {row}: max |device - restatement| = {err.max()} units, bound row 0 (max {want[:, 0].max()})")
        assert np.all(err <= want[:, 0]), (what, "row", row, int(err.max()))
    assert np.array_equal(per.sum(0), tot), (what, "summed output")


@pytest.mark.parametrize("n_mol", SIZES)
def test_against_the_restatement(n_mol):
    a = truncated(n_mol)
    box, R = a["box"], 3
    with make_batch(a, R) as b:
        diversify(b, a, seed=40 + n_mol)
        for numbins in (1, 50):
            for r_max in (0.0, RCUT):                            # 0: bins of (L / 2) / numbins
                what = f"N {n_mol}, {numbins} bins, r_max {r_max}"
                want = want_rows(b, a["charge"], [box] * R, numbins, r_max)
                # the restatement's own fp64 noise stays inside the bound: the pair loop backwards
                assert np.array_equal(want, want_rows(b, a["charge"], [box] * R, numbins, r_max, reverse=True)), what
                per = b.orient_corr(numbins, r_max, per_replica=True)
                tot = b.orient_corr(numbins, r_max)
                check_against(per, tot, want, n_mol, what)
                if r_max == 0.0:
                    assert np.array_equal(per, b.orient_corr(numbins, box / 2, per_replica=True)), what
                sites = b.rdf_sites(numbins, r_max, per_replica=True)
                assert np.array_equal(per[:, 0, :-1], sites[:, 0].astype(np.int64)), (what, "rdf_sites (0,0)")
        if n_mol == 1:
            assert not b.orient_corr(50, per_replica=True).any()
        else:
            per = b.orient_corr(50, per_replica=True)
            assert per[:, 0, :-1].sum() > 0 and np.abs(per[:, 1:]).sum() > 0
            assert not np.array_equal(per[0], per[1])


@pytest.mark.parametrize("numbins", [479, 480, 908, 909, 1636])
def test_the_bin_counts_at_which_a_workgroup_loses_waves(numbins):
    """The thresholds and a wave's four 64-bit rows, 8 rs + nw 32 rs bytes with rs = numbins + 2, within
    65536: four waves up to 479 bins, two from 480 to 908, one from 909 to MMC_ORIENT_MAX_BINS.  Three
    blocks a replica, and with wave_wgs = 1 the waves of one workgroup cross replica boundaries."""
    assert [nb for nb in range(1, 1637) if (8 + 4 * 32) * (nb + 2) <= 65536][-1] == 479
    assert [nb for nb in range(1, 1637) if (8 + 2 * 32) * (nb + 2) <= 65536][-1] == 908
    assert (8 + 32) * (1636 + 2) <= 65536 < (8 + 32) * (1637 + 2)
    n_mol, R = 129, 3
    a = truncated(n_mol)
    with make_batch(a, R) as b:
        diversify(b, a, seed=9)
        want = want_rows(b, a["charge"], [a["box"]] * R, numbins, RCUT)
        for wgs in (1, 0):
            b.set_option("wave_wgs", wgs)
            check_against(b.orient_corr(numbins, RCUT, per_replica=True), b.orient_corr(numbins, RCUT), want, n_mol,
                          f"{numbins} bins, wave_wgs {wgs}")


def test_molecules_that_differ_take_the_array_path():
    """A system whose molecules carry different charges has no 128-byte records: the kernel's other
    instantiation, reading the coordinate arrays."""
    box, n_mol, R = 22.0, 70, 2
    a = common.random_system(n_mol, box, seed=77, na_choices=(3,))
    with make_batch(a, R) as b:
        diversify(b, a, seed=5)
        for numbins, r_max in ((50, 0.0), (7, RCUT)):
            want = want_rows(b, a["charge"], [box] * R, numbins, r_max)
            check_against(b.orient_corr(numbins, r_max, per_replica=True), b.orient_corr(numbins, r_max), want,
                          n_mol, f"ragged charges, {numbins} bins")


def test_per_replica_boxes():
    a = truncated(70)
    factors = (1.0, 1.01, 1.03)
    with make_batch(a, 3, RCUT_PB) as b:
        diversify(b, a, seed=33)
        for r, f in enumerate(factors):      # every replica's own configuration, scaled to its box
            com, coords, _ = b.get_replica(r)
            b.set_replica(r, com * f, coords + np.repeat(com * f - com, 3, axis=0))
        b.set_boxes([a["box"] * f for f in factors], ALPHA)
        boxes = b.get_boxes()
        assert np.array_equal(boxes, [a["box"] * f for f in factors])
        for numbins in (1, 50):
            want = want_rows(b, a["charge"], boxes, numbins, RCUT_PB)      # r_cut = half of the smallest box
            per = b.orient_corr(numbins, RCUT_PB, per_replica=True)
            tot = b.orient_corr(numbins, RCUT_PB)
            check_against(per, tot, want, 70, f"per box, {numbins} bins")
            assert np.array_equal(per[:, 0, :-1],
                                  b.rdf_sites(numbins, RCUT_PB, per_replica=True)[:, 0].astype(np.int64))
        assert not np.array_equal(per[0, 0], per[2, 0])          # the boxes matter


def test_the_launch_does_not_change_a_bit():
    a = truncated(129)
    R = 3
    with make_batch(a, R) as b:
        diversify(b, a, seed=9)
        base = b.orient_corr(50, RCUT, per_replica=True)
        base_tot = b.orient_corr(50, RCUT)
        assert base.tobytes() == b.orient_corr(50, RCUT, per_replica=True).tobytes()      # two calls in a row
        assert base_tot.tobytes() == b.orient_corr(50, RCUT).tobytes()
        for wgs in (1, 2, 5):
            b.set_option("wave_wgs", wgs)      # 1: four waves share 18 tiles and cross replica boundaries
            assert b.orient_corr(50, RCUT, per_replica=True).tobytes() == base.tobytes(), wgs
            assert b.orient_corr(50, RCUT).tobytes() == base_tot.tobytes(), wgs
        # fewer waves per workgroup (their rows beside the thresholds in 64 KB): 2, then 1
        for numbins in (500, 1000, 1636):
            b.set_option("wave_wgs", 0)
            wide = b.orient_corr(numbins, RCUT, per_replica=True)
            b.set_option("wave_wgs", 1)
            assert b.orient_corr(numbins, RCUT, per_replica=True).tobytes() == wide.tobytes(), numbins
            assert np.array_equal(wide[:, :, :-1].sum(-1), base[:, :, :-1].sum(-1)), numbins
            assert np.array_equal(wide[:, :, -1], base[:, :, -1]), numbins


def test_sum_rule():
    """sum_{i<j} u_i.u_j = (|sum_i u_i|^2 - N') / 2 with N' the molecules that have an axis: row 1
    over all slots, the one beyond r_max included.  Tolerance: half a unit of rounding per pair on
    each side of the factor 2, plus the fp64 summation of the host's side."""
    n_mol = 129
    a = truncated(n_mol)
    with make_batch(a, 3) as b:
        diversify(b, a, seed=21)
        per = b.orient_corr(50, RCUT, per_replica=True)
        for r in range(3):
            com, coords, _ = b.get_replica(r)
            u = oref.axes(com, coords, a["charge"], a["box"])
            n_axis = int(np.any(u != 0.0, axis=1).sum())
            tot = u.sum(0)
            lhs = 2.0 * float(per[r, 1].sum()) / UNIT + n_axis
            tol = n_mol * (n_mol - 1) / 2 * 2.0 ** -30 + 1e-9 * n_mol
            print(f"replica {r}: 2 sum row1 / 2^30 + N' = {lhs!r}, |sum u|^2 = {float(tot @ tot)!r}, tol {tol:.3e}")
            assert n_axis == n_mol and abs(lhs - float(tot @ tot)) <= tol, r
            gk = _kirkwood(per[r], n_mol)
            assert abs(gk[-1] - float(tot @ tot) / n_mol) <= tol / n_mol


def _kirkwood(hist, n_mol):
    from metropolismontecarlo_amd import observables
    return observables.kirkwood_gk(hist, n_mol)


@pytest.mark.parametrize("style", ["ewald", "wolf"])
def test_the_call_is_read_only(style):
    a = common.nist_arrays(1, "unwrapped")
    R, runs = 3, []
    for watched in (False, True):
        with make_batch(a, R) as b:
            b.set_option("device_moves", 1)
            if style == "wolf":
                b.set_coulomb_style("wolf")
                total = b.potential_wolf
            else:
                total = b.potential_ewald
            e = total(as_array=True)["energy"].copy()
            if watched:
                before = [b.get_replica(r) for r in range(R)]
                b.orient_corr(50, RCUT, per_replica=True)
                for x, y in zip(before, [b.get_replica(r) for r in range(R)]):
                    assert all(u.tobytes() == v.tobytes() for u, v in zip(x, y))
                assert total(as_array=True).tobytes() == total(as_array=True).tobytes()
            e, st1 = b.run(60, T, DR, DPHI, seed=17, energies=e)
            if watched:
                b.orient_corr(50, RCUT, per_replica=True)
                b.orient_corr(20)
            e, st2 = b.run(60, T, DR, DPHI, seed=18, energies=e)
            runs.append((e, [{k: v for k, v in st.items() if isinstance(v, int)} for st in (st1, st2)],
                         [b.get_replica(r) for r in range(R)], total(as_array=True).copy()))
    plain, seen = runs
    assert plain[0].tobytes() == seen[0].tobytes()                    # the running energies
    assert plain[1] == seen[1]
    for x, y in zip(plain[2], seen[2]):                               # coordinates and S(k)
        assert all(u.tobytes() == v.tobytes() for u, v in zip(x, y))
    assert plain[3].tobytes() == seen[3].tobytes()                    # the recomputed totals
    assert plain[1][0]["moves"] == R * 60


def test_refusals_leave_hist_untouched():
    a = truncated(70)
    R, box = 2, a["box"]
    sentinel = -0x0123456789abcdef

    def expect(status, b, numbins=10, r_max=0.0, per=False):
        n2 = max(numbins, 0) + 2
        h = np.full((R, 4, n2) if per else (4, n2), sentinel, dtype=np.int64)
        with pytest.raises(_lib.MMCError) as ei:
            b.orient_corr(numbins, r_max, per_replica=per, out=h)
        assert ei.value.status == status and np.all(h == sentinel), (numbins, r_max, per)

    with make_batch(a, R, RCUT_PB) as b:
        # proposals outstanding
        b.eval(np.full(R, 3), np.tile(a["com"][2], (R, 1)), np.tile(a["coords"][6:9], (R, 1, 1)))
        expect(_lib.MMC_ERR_STATE, b)
        expect(_lib.MMC_ERR_STATE, b, per=True)
        expect(_lib.MMC_ERR_ARG, b, numbins=0)                    # arguments come before the state
        b.settle(np.zeros(R, dtype=np.int32))
        for r_max in (np.nextafter(box / 2, 100.0), box, float("nan"), float("inf")):
            expect(_lib.MMC_ERR_ARG, b, r_max=r_max)
            expect(_lib.MMC_ERR_ARG, b, r_max=r_max, per=True)
        for nb in (0, -3, 1637, 5000):                            # MMC_ORIENT_MAX_BINS = 1636
            expect(_lib.MMC_ERR_ARG, b, numbins=nb)
        assert _lib.lib().mmc_batch_orient_corr(b._h, 10, 0.0, 0, None) == _lib.MMC_ERR_ARG
        # ... and after all that the call works, r_max = L / 2 exactly and the largest numbins included
        assert np.array_equal(b.orient_corr(10, box / 2), b.orient_corr(10))
        assert b.orient_corr(1636, RCUT)[0].sum() == R * 70 * 69 // 2
        # per-replica boxes: no common L / 2, and half of the SMALLEST box bounds r_max
        b.set_boxes([box, 1.02 * box], ALPHA)
        boxes = b.get_boxes()
        for r_max in (0.0, -1.0, np.nextafter(0.5 * boxes.min(), 100.0), 0.5 * boxes.max()):
            expect(_lib.MMC_ERR_ARG, b, r_max=r_max)
            expect(_lib.MMC_ERR_ARG, b, r_max=r_max, per=True)
        # a volume trial in flight
        b.volume_trial_replicas(boxes * np.array([1.01, 0.0]))
        expect(_lib.MMC_ERR_STATE, b, r_max=RCUT)
        expect(_lib.MMC_ERR_ARG, b, r_max=0.0)
        b.volume_settle(np.zeros(R, dtype=np.int32))
        assert b.orient_corr(10, RCUT)[0].sum() == R * 70 * 69 // 2
