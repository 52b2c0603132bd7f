"""mmc_batch_pair_energy against its numpy restatement (tests/pair_energy_ref.py) on SPC/E molecules of
the NIST fixtures, truncated to the sizes at which k_pair_energy_wave takes another path.

Launch shape: k_orient_corr_wave's.  The unit is a 64 x 64 tile of the i < j triangle, K (K + 1) / 2 per
replica with K = ceil(N / 64); wave W of the launch's NW takes the contiguous run
[n_tiles W / NW, n_tiles (W + 1) / NW).  N = 1, 2, 63, 64, 70 and 129 are the smallest sizes with an
empty triangle, one pair, a partial block, a full block, a half-masked diagonal tile and an
off-diagonal tile; with option wave_wgs = 1 four waves share the 18 tiles of three replicas of 129
molecules, so a wave crosses replica boundaries and flushes its LDS counters and the neighbour side's
register count in between.

Bounds.  Row 0, uhist, nhb and flagged are exact -- once the restatement itself is clear of every
decision: the device may evaluate u_C and u_LJ of an unflagged pair within 2^-21 K of the restatement
(include/mmc_hip.h), so every test first asserts that no unflagged pair lies within 2^-20 K of an
energy-bin edge, of u_hb or of the 2^20 K flag limit.  Rows 1 and 2: two values within 2^-21 K round to
integers at most 1 apart and each pair contributes once: per slot |device - restatement| <= row 0 of
that slot, in units."""
import numpy as np
import pytest

import common
import pair_energy_ref as pref
from metropolismontecarlo_amd import _lib, structs
from test_gpu_orient import ALPHA, RCUT, RCUT_PB, diversify, make_batch, truncated

pytestmark = pytest.mark.gpu

T, DR, DPHI = 298.15, 0.3, 0.2
SIZES = (1, 2, 63, 64, 70, 129)
E_BINS, U_LO, U_HI, U_HB = 60, -4000.0, 2000.0, -1132.2
CLEAR = 2.0 ** -20
MAX_BINS = 1016                  # MMC_PAIRE_MAX_BINS


def want_all(b, a, boxes, numbins, r_max, reverse=False, n_ebins=E_BINS, u_lo=U_LO, u_hi=U_HI, u_hb=U_HB):
    """The restatement of every replica from the batch's own coordinates, each replica at its box."""
    out = []
    for r in range(b.R):
        _, coords, _ = b.get_replica(r)
        out.append(pref.pair_energy(coords, a["atype"], a["charge"], a["eps"], a["sig"], structs.factor,
                                    float(boxes[r]), numbins, r_max, n_ebins, u_lo, u_hi, u_hb, reverse=reverse))
    return out


def precondition(want, what):
    for r, w in enumerate(want):
        m = w["margins"]
        print(f"{what} replica {r}: closest to a bin edge {m['edge']:.3e} K, to u_hb {m['hb']:.3e} K, "
              f"to the 2^20 limit {m['limit']:.3e} K")
        assert m["edge"] > CLEAR and m["hb"] > CLEAR and m["limit"] > CLEAR, (what, r, m)


def check_against(per, tot, want, n_mol, what):
    """per, tot: PairEnergy of a per-replica and a summed call; want: want_all's list."""
    R = len(want)
    rows = np.stack([w["rows"] for w in want])
    assert per.rows.dtype == np.int64 and per.rows.shape == rows.shape and tot.rows.shape == rows.shape[1:], what
    assert np.array_equal(per.rows[:, 0], rows[:, 0]), (what, "row 0")
    assert np.all(per.rows[:, 0].sum(-1) == n_mol * (n_mol - 1) // 2), what
    assert np.all(per.rows[:, 1:, -1] == 0), (what, "rows 1 and 2 beyond r_max")
    for row in (1, 2):
        err = np.abs(per.rows[:, row] - rows[:, row])
        print(f"{what} row {row}: max |device - restatement| = {err.max()} units, bound row 0 (max {rows[:, 0].max()})")
        assert np.all(err <= rows[:, 0]), (what, "row", row, int(err.max()))
    flagged = np.array([w["flagged"] for w in want], dtype=np.uint64)
    assert per.flagged.dtype == np.uint64 and np.array_equal(per.flagged, flagged), (what, "flagged")
    assert np.array_equal(per.rows.sum(0), tot.rows) and tot.flagged.shape == (1,) and tot.flagged[0] == flagged.sum(), what
    if per.uhist is not None:
        uhist = np.stack([w["uhist"] for w in want])
        assert per.uhist.dtype == np.uint64 and np.array_equal(per.uhist, uhist), (what, "uhist")
        assert np.array_equal(per.uhist.sum(0), tot.uhist), (what, "summed uhist")
        assert np.array_equal(per.uhist.sum(-1), per.rows[:, 0, :-1].sum(-1).astype(np.uint64) - flagged), what
    if per.nhb is not None:
        nhb = np.stack([w["nhb"] for w in want])
        assert per.nhb.dtype == np.uint64 and np.array_equal(per.nhb, nhb), (what, "nhb")
        assert np.array_equal(per.nhb.sum(0), tot.nhb), (what, "summed nhb")
        assert np.all(per.nhb.sum(-1) == n_mol), (what, "sum nhb")
        for r, w in enumerate(want):
            if w["cnt"].max(initial=0) <= pref.NHB - 1:              # no molecule saturates the last slot
                assert int((per.nhb[r] * np.arange(pref.NHB, dtype=np.uint64)).sum()) == 2 * w["n_below"], (what, r)
    return flagged


def both(b, numbins, r_max, **kw):
    kw = dict(dict(n_ebins=E_BINS, u_lo=U_LO, u_hi=U_HI, u_hb=U_HB), **kw)
    return b.pair_energy(numbins, r_max, per_replica=True, **kw), b.pair_energy(numbins, r_max, **kw)


def same(x, y):
    return all((u is None and v is None) or u.tobytes() == v.tobytes() for u, v in zip(x, y))


@pytest.mark.parametrize("n_mol", SIZES)
def test_against_the_restatement(n_mol):
    a = truncated(n_mol)
    box, R = a["box"], 3
    with make_batch(a, R) as b:
        diversify(b, a, seed=40 + n_mol)
        for numbins in (1, 50):
            for r_max in (0.0, RCUT):                            # 0: bins of (L / 2) / numbins
                what = f"N {n_mol}, {numbins} bins, r_max {r_max}"
                want = want_all(b, a, [box] * R, numbins, r_max)
                precondition(want, what)
                # the restatement's own fp64 noise stays inside the bound: the pair loop backwards
                back = want_all(b, a, [box] * R, numbins, r_max, reverse=True)
                for w, v in zip(want, back):
                    assert all(np.array_equal(w[k], v[k]) for k in ("rows", "uhist", "nhb", "cnt")), what
                    assert w["flagged"] == v["flagged"]
                per, tot = both(b, numbins, r_max)
                flagged = check_against(per, tot, want, n_mol, what)
                assert not flagged.any(), what                   # the NIST configurations flag nothing
                if r_max == 0.0:
                    assert same(per, b.pair_energy(numbins, box / 2, E_BINS, U_LO, U_HI, U_HB, per_replica=True)), what
                orient = b.orient_corr(numbins, r_max, per_replica=True)
                assert np.array_equal(per.rows[:, 0], orient[:, 0]), (what, "orient_corr row 0")
        if n_mol == 1:
            per, tot = both(b, 50, 0.0)
            assert not per.rows.any() and not per.uhist.any() and not per.flagged.any()
            assert np.array_equal(per.nhb, np.tile([1] + [0] * 8, (R, 1)).astype(np.uint64))
        elif n_mol >= 63:
            per, tot = both(b, 50, 0.0)
            assert per.rows[:, 0, :-1].sum() > 0 and np.abs(per.rows[:, 1:]).sum() > 0 and per.nhb[:, 1:].sum() > 0
            assert not np.array_equal(per.rows[0], per.rows[1])


def wave_boundaries(n_ebins):
    """The numbins at which a workgroup of k_pair_energy_wave loses waves, from the header's limits: the
    thresholds, the 144 bytes of LJ constants and a wave's 3 rs + e_slots + 1 64-bit counters,
    8 rs + 144 + nw 8 (3 rs + e_slots + 1) bytes with rs = numbins + 2, within 65536.  For nw = 4 and 2:
    the last numbins that fits and the first that does not, where the call allows them; then the
    largest numbins allowed."""
    from common import header_define
    max_bins, max_ebins = int(header_define("MMC_PAIRE_MAX_BINS")), int(header_define("MMC_PAIRE_MAX_EBINS"))
    assert max_bins == MAX_BINS and n_ebins <= max_ebins
    e_slots = n_ebins + 2 if n_ebins else 0

    def fits(nw, nb):
        return 8 * (nb + 2) + 144 + nw * 8 * (3 * (nb + 2) + e_slots + 1) <= 65536
    assert fits(1, max_bins) and (n_ebins < max_ebins or not fits(1, max_bins + 1))
    out = set()
    for nw in (4, 2):
        last = max([nb for nb in range(1, max_bins + 1) if fits(nw, nb)], default=0)
        out |= {nb for nb in (last, last + 1) if 1 <= nb <= max_bins}
    return sorted(out | {max_bins})


# without uhist: four waves up to 626 bins, two beyond (MMC_PAIRE_MAX_BINS is below the 1165 that two
# waves hold); with the largest energy histogram one wave from the first bin on
@pytest.mark.parametrize("n_ebins,numbins", [(0, 626), (0, 627), (0, MAX_BINS), (4096, 1), (4096, MAX_BINS)])
def test_the_bin_counts_at_which_a_workgroup_loses_waves(n_ebins, numbins):
    assert wave_boundaries(0) == [626, 627, MAX_BINS] and wave_boundaries(4096) == [1, MAX_BINS]
    n_mol, R = 129, 3
    a = truncated(n_mol)
    with make_batch(a, R) as b:
        diversify(b, a, seed=40 + 129)
        what = f"{numbins} bins, {n_ebins} energy bins"
        want = want_all(b, a, [a["box"]] * R, numbins, RCUT, n_ebins=max(n_ebins, 1))
        precondition(want, what)
        for wgs in (1, 0):
            b.set_option("wave_wgs", wgs)
            per, tot = both(b, numbins, RCUT, n_ebins=n_ebins)
            assert (per.uhist is None) == (n_ebins == 0)
            check_against(per, tot, want, n_mol, f"{what}, wave_wgs {wgs}")


def test_outputs_that_are_not_asked_for_and_the_edges_of_the_arguments():
    n_mol, R = 70, 3
    a = truncated(n_mol)
    box = a["box"]
    with make_batch(a, R) as b:
        diversify(b, a, seed=3)
        full = both(b, 50, RCUT)
        # uhist and nhb NULL, each alone and both
        for kw in (dict(n_ebins=0), dict(u_hb=None), dict(n_ebins=0, u_hb=None)):
            per, tot = both(b, 50, RCUT, **kw)
            assert (per.uhist is None) == ("n_ebins" in kw) and (per.nhb is None) == ("u_hb" in kw)
            for got, ref in ((per, full[0]), (tot, full[1])):
                assert got.rows.tobytes() == ref.rows.tobytes() and got.flagged.tobytes() == ref.flagged.tobytes()
                assert got.uhist is None or got.uhist.tobytes() == ref.uhist.tobytes()
                assert got.nhb is None or got.nhb.tobytes() == ref.nhb.tobytes()
        # u_hb = u_hi: every unflagged pair below the top of the histogram counts as a bond
        want = want_all(b, a, [box] * R, 50, RCUT, u_hb=U_HI)
        precondition(want, "u_hb = u_hi")
        per, tot = both(b, 50, RCUT, u_hb=U_HI)
        check_against(per, tot, want, n_mol, "u_hb = u_hi")
        assert np.array_equal(per.uhist[:, :-1].sum(-1), np.array([w["n_below"] for w in want], dtype=np.uint64))
        # one energy bin, and the largest numbins (one wave per workgroup)
        want = want_all(b, a, [box] * R, MAX_BINS, RCUT, n_ebins=1)
        precondition(want, "n_ebins 1")
        per, tot = both(b, MAX_BINS, RCUT, n_ebins=1)
        check_against(per, tot, want, n_mol, f"{MAX_BINS} bins, 1 energy bin")
        assert per.uhist.shape == (R, 3)
        assert np.array_equal(per.rows[:, :, :-1].sum(-1), full[0].rows[:, :, :-1].sum(-1))
        assert np.array_equal(per.nhb, full[0].nhb)
        # the largest energy histogram beside it
        per, tot = both(b, MAX_BINS, RCUT, n_ebins=4096)
        assert np.array_equal(per.uhist.sum(-1), full[0].uhist.sum(-1)) and np.array_equal(per.uhist.sum(0), tot.uhist)
        # `out` is overwritten and returned
        out = dict(rows=np.full((3, 52), 7, dtype=np.int64), flagged=np.full(1, 7, dtype=np.uint64),
                   uhist=np.full(E_BINS + 2, 7, dtype=np.uint64), nhb=np.full(9, 7, dtype=np.uint64))
        got = b.pair_energy(50, RCUT, E_BINS, U_LO, U_HI, U_HB, out=out)
        assert got.rows is out["rows"] and got.uhist is out["uhist"] and got.nhb is out["nhb"]
        assert same(got, full[1])


def test_molecules_that_differ_take_the_array_path_and_overlaps_are_flagged():
    """A system whose molecules carry different charges and atom types has no 128-byte records: the
    kernel's other instantiation, reading the coordinate arrays and the eps / sig tables by type.
    Molecule 5 lies exactly on molecule 4 (r = 0: not finite) and molecule 7 half an angstrom from
    molecule 6 (beyond 2^20 K)."""
    box, n_mol, R = 22.0, 70, 2
    a = common.random_system(n_mol, box, seed=77, na_choices=(3,))
    com, coords = a["com"].copy(), a["coords"].copy()
    com[5], coords[15:18] = com[4], coords[12:15]
    com[7], coords[21:24] = com[6] + [0.5, 0.0, 0.0], coords[18:21] + [0.5, 0.0, 0.0]
    a = dict(a, com=com, coords=coords)
    with make_batch(a, R) as b:
        diversify(b, a, seed=5)
        for numbins, r_max in ((50, 0.0), (7, RCUT)):
            what = f"ragged molecules, {numbins} bins"
            want = want_all(b, a, [box] * R, numbins, r_max)
            precondition(want, what)
            per, tot = both(b, numbins, r_max)
            flagged = check_against(per, tot, want, n_mol, what)
            assert flagged[0] >= 2 and tot.flagged[0] > 0, flagged
            assert np.array_equal(per.rows[:, 0], b.orient_corr(numbins, r_max, per_replica=True)[:, 0])


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
            what = f"per box, {numbins} bins"
            want = want_all(b, a, boxes, numbins, RCUT_PB)           # r_cut = half of the smallest box
            precondition(want, what)
            per, tot = both(b, numbins, RCUT_PB)
            assert not check_against(per, tot, want, 70, what).any()
            assert np.array_equal(per.rows[:, 0], b.orient_corr(numbins, RCUT_PB, per_replica=True)[:, 0])
        assert not np.array_equal(per.rows[0, 0], per.rows[2, 0])    # the boxes matter


def test_the_launch_does_not_change_a_bit():
    a = truncated(129)
    R = 3
    with make_batch(a, R) as b:
        diversify(b, a, seed=40 + 129)       # (test_against_the_restatement checks these values at the default grid)
        base = both(b, 50, RCUT)
        again = both(b, 50, RCUT)
        assert same(base[0], again[0]) and same(base[1], again[1])           # two calls in a row
        for wgs in (1, 2, 5):
            b.set_option("wave_wgs", wgs)    # 1: four waves share 18 tiles and cross replica boundaries
            got = both(b, 50, RCUT)
            assert same(base[0], got[0]) and same(base[1], got[1]), wgs
        # fewer waves per workgroup (their counters beside the thresholds in 64 KB): four, two, two, and one
        # with the largest energy histogram as well
        for numbins, n_ebins in ((400, E_BINS), (800, E_BINS), (MAX_BINS, E_BINS), (MAX_BINS, 4096)):
            b.set_option("wave_wgs", 0)
            wide = both(b, numbins, RCUT, n_ebins=n_ebins)
            b.set_option("wave_wgs", 1)
            got = both(b, numbins, RCUT, n_ebins=n_ebins)
            assert same(wide[0], got[0]) and same(wide[1], got[1]), numbins
            assert np.array_equal(wide[0].rows[:, :, :-1].sum(-1), base[0].rows[:, :, :-1].sum(-1)), numbins
            assert wide[0].nhb.tobytes() == base[0].nhb.tobytes()
            assert np.array_equal(wide[0].uhist.sum(-1), base[0].uhist.sum(-1))
            if n_ebins == E_BINS:
                assert wide[0].uhist.tobytes() == base[0].uhist.tobytes()


@pytest.mark.parametrize("style", ["ewald", "wolf"])
def test_the_call_is_read_only_and_the_same_in_either_style(style):
    a = common.nist_arrays(1, "unwrapped")
    R = 3
    with make_batch(a, R) as b:
        diversify(b, a, seed=11)
        ewald = both(b, 50, RCUT)
        if style == "wolf":
            b.set_coulomb_style("wolf")
            total = b.potential_wolf
        else:
            total = b.potential_ewald
        e0 = total(as_array=True).copy()                                     # (refreshes S(k) after diversify)
        before = [b.get_replica(r) for r in range(R)]
        got = both(b, 50, RCUT)
        assert same(ewald[0], got[0]) and same(ewald[1], got[1])             # the bare pair energy in both styles
        for x, y in zip(before, [b.get_replica(r) for r in range(R)]):       # coordinates and S(k)
            assert all(u.tobytes() == v.tobytes() for u, v in zip(x, y))
        assert total(as_array=True).tobytes() == e0.tobytes()
        # a chain goes on as if nothing had been asked
        b.set_option("device_moves", 1)
        e, st = b.run(40, T, DR, DPHI, seed=17, energies=e0["energy"].copy())
        assert st["moves"] == R * 40 and np.all(np.isfinite(e))
        both(b, 20, 0.0)


def test_refusals_leave_every_output_untouched():
    a = truncated(70)
    R, box = 2, a["box"]
    sentinel = 0x0123456789abcdef

    def expect(status, b, numbins=10, r_max=0.0, per=False, **kw):
        kw = dict(dict(n_ebins=E_BINS, u_lo=U_LO, u_hi=U_HI, u_hb=U_HB), **kw)
        lead = (R,) if per else ()
        out = dict(rows=np.full(lead + (3, max(numbins, 0) + 2), sentinel, dtype=np.int64),
                   flagged=np.full(lead if per else (1,), sentinel, dtype=np.uint64))
        if kw["n_ebins"] != 0:
            out["uhist"] = np.full(lead + (max(kw["n_ebins"], 0) + 2,), sentinel, dtype=np.uint64)
        if kw["u_hb"] is not None:
            out["nhb"] = np.full(lead + (9,), sentinel, dtype=np.uint64)
        with pytest.raises(_lib.MMCError) as ei:
            b.pair_energy(numbins, r_max, per_replica=per, out=out, **kw)
        assert ei.value.status == status and all(np.all(v == sentinel) for v in out.values()), (numbins, r_max, per, kw)

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
        for nb in (0, -3, MAX_BINS + 1, 5000):
            expect(_lib.MMC_ERR_ARG, b, numbins=nb)
        for kw in (dict(n_ebins=-1), dict(n_ebins=4097), dict(u_lo=U_HI), dict(u_hi=float("nan")),
                   dict(u_hb=float("inf")), dict(u_hb=float("nan"))):
            expect(_lib.MMC_ERR_ARG, b, **kw)
            expect(_lib.MMC_ERR_ARG, b, per=True, **kw)
        # ... and after all that the call works, r_max = L / 2 exactly included
        assert same(b.pair_energy(10, box / 2, E_BINS, U_LO, U_HI, U_HB), b.pair_energy(10, 0.0, E_BINS, U_LO, U_HI, U_HB))
        assert b.pair_energy(MAX_BINS, RCUT).rows[0].sum() == R * 70 * 69 // 2
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
        assert b.pair_energy(10, RCUT).rows[0].sum() == R * 70 * 69 // 2
