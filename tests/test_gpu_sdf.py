"""mmc_batch_sdf against its numpy restatement (tests/sdf_ref.py), integer for integer, on SPC/E
molecules of the NIST fixtures truncated to the sizes at which k_sdf_wave takes another path.

Launch shape: the unit is mmc_tiles.hpp's 64 x 64 tile of the i < j triangle, K (K + 1) / 2 per
replica with K = ceil(N / 64); workgroup B of the launch's G takes the contiguous run
[n_tiles B / G, n_tiles (B + 1) / G), cuts it where the replica changes (per-replica output) and its
waves share each segment.  N = 70 and 129 are the smallest sizes with a partial last block, a
half-masked diagonal tile and an off-diagonal tile; with option wave_wgs = 1 one workgroup walks the
18 tiles of three replicas of 129 molecules and flushes its grid at both boundaries.  The grid of
the workgroup lives in LDS: up to 40 KB four workgroups of 4 waves share a compute unit, up to 80 KB
two of 8, beyond that one of 16, and above 64 KB the kernel opts in to large dynamic LDS."""
import numpy as np
import pytest

import common
import sdf_ref as sref
from metropolismontecarlo_amd import _lib
from test_gpu_orient import ALPHA, RCUT_PB, diversify, make_batch, truncated

pytestmark = pytest.mark.gpu

T, DR, DPHI = 298.15, 0.3, 0.2
SIZES = (1, 2, 63, 64, 70, 129)
N_HALF, CELL = 8, 0.5              # sqrt(3) 4 + rho = 8.9 <= L / 2 = 10 with rho = 2 r_mol_max < 2 A


def want_counts(b, boxes, n_half, cell, fold, mask):
    """[R, cells + 2] from the batch's own coordinates, each replica at its box."""
    return np.stack([sref.sdf_counts(b.get_replica(r)[1], float(boxes[r]), n_half, cell, fold, mask)
                     for r in range(b.R)])


def flat(res):
    """An Sdf result back in the library's layout [..., cells + 2]."""
    lead = res.outside.shape
    return np.concatenate([res.grid.reshape(lead + (-1,)), res.outside[..., None], res.noframe[..., None]], axis=-1)


def check_against(b, want, n_mol, n_half, cell, fold, mask, what):
    per = b.sdf(n_half, cell, fold, mask, per_replica=True)
    tot = b.sdf(n_half, cell, fold, mask)
    shape = sref.grid_shape(n_half, fold)
    assert per.grid.dtype == np.uint64 and per.grid.shape == (b.R,) + shape and tot.grid.shape == shape, what
    assert per.outside.shape == (b.R,) and tot.outside.shape == (), what
    got = flat(per)
    diff = np.argwhere(got != want)
    assert diff.size == 0, (what, "first differences", diff[:5].tolist(), got[got != want][:5], want[got != want][:5])
    assert np.all(got.sum(-1) == n_mol * (n_mol - 1) * bin(mask).count("1")), (what, "sum rule")
    assert np.array_equal(flat(tot), got.sum(0)), (what, "summed output")
    return per


@pytest.mark.parametrize("n_mol", SIZES)
def test_against_the_restatement(n_mol):
    a = truncated(n_mol)
    box, R = a["box"], 3
    with make_batch(a, R) as b:
        diversify(b, a, seed=60 + n_mol)
        for fold in (0, 3):
            for mask in (1, 6, 7):
                what = f"N {n_mol}, fold {fold}, site_mask {mask}"
                want = want_counts(b, [box] * R, N_HALF, CELL, fold, mask)
                per = check_against(b, want, n_mol, N_HALF, CELL, fold, mask, what)
                assert not per.noframe.any(), what
        if n_mol == 1:
            assert not flat(b.sdf(N_HALF, CELL, per_replica=True)).any()
        elif n_mol > 2:
            per = b.sdf(N_HALF, CELL, per_replica=True)
            assert per.grid.sum() > 0 and per.outside.sum() > 0
            assert not np.array_equal(per.grid[0], per.grid[1])
        # a one-cell half-axis
        for fold in (0, 3):
            want = want_counts(b, [box] * R, 1, 3.5, fold, 7)
            check_against(b, want, n_mol, 1, 3.5, fold, 7, f"N {n_mol}, n_half 1, fold {fold}")


def test_the_fullest_cell_of_the_fixture():
    """The acceptor oxygen in front of a hydrogen (tests/test_sdf_host.py): replica 0 is the fixture."""
    a = truncated(129)
    with make_batch(a, 2) as b:
        g = b.sdf(N_HALF, CELL, per_replica=True).grid[0]
        assert np.unravel_index(np.argmax(g), g.shape) == (4, 0, 11) and g[4, 0, 11] == 48


def test_replica_crossings():
    """wave_wgs = 1: one workgroup's run crosses both replica boundaries; 2 and 5: the boundaries fall
    inside and between the workgroups' runs.  Per-replica output stays exact and equals the default
    grid's; two calls agree bit for bit."""
    n_mol, R = 129, 3
    a = truncated(n_mol)
    with make_batch(a, R) as b:
        diversify(b, a, seed=9)
        want = want_counts(b, [a["box"]] * R, N_HALF, CELL, 3, 7)
        base = flat(check_against(b, want, n_mol, N_HALF, CELL, 3, 7, "default grid"))
        assert base.tobytes() == flat(b.sdf(N_HALF, CELL, 3, 7, per_replica=True)).tobytes()
        for wgs in (1, 2, 5):
            b.set_option("wave_wgs", wgs)
            got = flat(check_against(b, want, n_mol, N_HALF, CELL, 3, 7, f"wave_wgs {wgs}"))
            assert got.tobytes() == base.tobytes(), wgs


@pytest.mark.parametrize("n_half,cell,fold", [
    (16, 0.25, 0),      # 32768 cells: MMC_SDF_MAX_CELLS, 128 KB, one workgroup of 16 waves per compute unit
    (16, 0.25, 1),      # 16384 cells: 65536 + 264 bytes, just above what needs no opting in (two workgroups of 8)
    (20, 0.2, 3),       # 16000 cells: 64000 + 328 bytes, just below
    (13, 0.3, 3),       # 4394 cells: 17576 + 216 bytes (four workgroups of 4 waves)
], ids=["128KB", "above-64KB", "below-64KB", "small"])
def test_the_grid_sizes_at_which_the_workgroup_changes(n_half, cell, fold):
    lds = 8 * (2 * n_half + 1) + 4 * int(np.prod(sref.grid_shape(n_half, fold)))
    assert {(16, 0): lds == 131336, (16, 1): 65536 < lds <= 81920, (20, 3): 40960 < lds <= 65536,
            (13, 3): lds <= 40960}[(n_half, fold)]
    n_mol, R = 129, 3
    a = truncated(n_mol)
    with make_batch(a, R) as b:
        diversify(b, a, seed=9)
        want = want_counts(b, [a["box"]] * R, n_half, cell, fold, 7)
        for wgs in (0, 1):
            b.set_option("wave_wgs", wgs)
            check_against(b, want, n_mol, n_half, cell, fold, 7, f"n_half {n_half}, fold {fold}, wave_wgs {wgs}")


def test_molecules_that_differ_take_the_array_path():
    """A system whose molecules carry different charges has no 128-byte records: the kernel's other
    instantiation, reading the coordinate arrays."""
    box, n_mol, R = 22.0, 70, 2
    a = common.random_system(n_mol, box, seed=77, na_choices=(3,))
    with make_batch(a, R) as b:
        diversify(b, a, seed=5)
        for fold, mask in ((3, 1), (0, 7)):
            want = want_counts(b, [box] * R, 6, 0.5, fold, mask)
            check_against(b, want, n_mol, 6, 0.5, fold, mask, f"ragged charges, fold {fold}, site_mask {mask}")


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
        for fold, mask in ((3, 7), (0, 1)):
            want = want_counts(b, boxes, N_HALF, CELL, fold, mask)
            per = check_against(b, want, 70, N_HALF, CELL, fold, mask, f"per box, fold {fold}")
        same = want_counts(b, [boxes[0]] * 3, N_HALF, CELL, 0, 1)
        assert not np.array_equal(same[2], flat(per)[2])            # the boxes matter


def test_centres_without_a_frame():
    """One linear and one collapsed molecule in replica 1: each sends its (N - 1) popcount(mask)
    deposits as a centre to noframe; as neighbours their sites are still deposited."""
    n_mol, R = 70, 3
    a = truncated(n_mol)
    with make_batch(a, R) as b:
        diversify(b, a, seed=12)
        com, coords, _ = b.get_replica(1)
        coords = coords.copy()
        for m in (5, 66):                      # site 0 on a dyadic position: the offsets below are exact
            coords[3 * m] = np.round(coords[3 * m] * 8.0) / 8.0
        o = coords[3 * 5]
        coords[3 * 5 + 1], coords[3 * 5 + 2] = o + (0.75, 0.25, 0.0), o - (0.75, 0.25, 0.0)      # o2 = -o1: b = 0
        o = coords[3 * 66]
        coords[3 * 66 + 1] = coords[3 * 66 + 2] = o + (0.5, 0.0, 0.5)                              # o1 = o2: h = 0
        b.set_replica(1, com, coords)
        got = b.get_replica(1)[1]
        ok = sref.frames(got, a["box"])[3]
        assert not ok[5] and not ok[66] and ok.sum() == n_mol - 2
        n_bad = 2
        for fold, mask in ((3, 1), (0, 6), (3, 7)):
            want = want_counts(b, [a["box"]] * R, N_HALF, CELL, fold, mask)
            per = check_against(b, want, n_mol, N_HALF, CELL, fold, mask, f"no frame, site_mask {mask}")
            assert per.noframe.tolist() == [0, n_bad * (n_mol - 1) * bin(mask).count("1"), 0]


def test_the_cube_against_the_periodic_images():
    """Refused when sqrt(3) n_half cell + 2 r_mol_max exceeds half of the smallest box.  r_mol_max of an
    undiversified batch is the uploaded configuration's: max |site - COM|."""
    a = truncated(70)
    R, box = 2, a["box"]
    d = a["coords"].reshape(-1, 3, 3) - a["com"][:, None, :]
    rho = 2.0 * float(np.sqrt(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).max()))
    assert 1.8 < rho < 2.0
    edge = (box / 2 - rho) / (np.sqrt(3.0) * N_HALF)         # the cell at which the cube just fits
    with make_batch(a, R, RCUT_PB) as b:
        for per in (False, True):
            res = b.sdf(N_HALF, edge * (1 - 1e-9), per_replica=per)
            assert res.grid.sum() + res.outside.sum() == R * 70 * 69
            with pytest.raises(_lib.MMCError) as ei:
                b.sdf(N_HALF, edge * (1 + 1e-9), per_replica=per)
            assert ei.value.status == _lib.MMC_ERR_ARG and "half of the smallest box" in str(ei.value)
        with pytest.raises(_lib.MMCError) as ei:
            b.sdf(17, 0.1, fold=0)                              # 8 x 17^3 cells > MMC_SDF_MAX_CELLS
        assert ei.value.status == _lib.MMC_ERR_ARG
        # per-replica boxes: the smallest one counts
        b.set_boxes([1.05 * box, 1.02 * box], ALPHA)
        small = (1.02 * box / 2 - rho) / (np.sqrt(3.0) * N_HALF)
        assert b.sdf(N_HALF, small * (1 - 1e-9)).grid.sum() > 0
        with pytest.raises(_lib.MMCError) as ei:
            b.sdf(N_HALF, small * (1 + 1e-9))
        assert ei.value.status == _lib.MMC_ERR_ARG


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
                b.sdf(N_HALF, CELL, 3, 7, per_replica=True)
                for x, y in zip(before, [b.get_replica(r) for r in range(R)]):
                    assert all(u.tobytes() == v.tobytes() for u, v in zip(x, y))
            e, st1 = b.run(60, T, DR, DPHI, seed=17, energies=e)
            if watched:
                per = b.sdf(N_HALF, CELL, 3, 7, per_replica=True)
                assert flat(per).tobytes() == flat(b.sdf(N_HALF, CELL, 3, 7, per_replica=True)).tobytes()
                want = want_counts(b, [a["box"]] * R, N_HALF, CELL, 3, 7)       # ... on coordinates a chain left
                assert np.array_equal(flat(per), want)
                b.sdf(16, 0.25, 0)
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
    R = 2
    sentinel = 0xfedcba9876543210

    def expect(status, b, per=False, **kw):
        cells = int(np.prod(sref.grid_shape(N_HALF, kw.get("fold", 3))))
        h = np.full((R, cells + 2) if per else (cells + 2,), sentinel, dtype=np.uint64)
        with pytest.raises(_lib.MMCError) as ei:
            b.sdf(N_HALF, kw.pop("cell", CELL), per_replica=per, out=h, **kw)
        assert ei.value.status == status and np.all(h == sentinel), (kw, per)

    with make_batch(a, R, RCUT_PB) as b:
        base = flat(b.sdf(N_HALF, CELL, per_replica=True))
        # a volume trial in flight
        boxes = np.array([a["box"]] * R)
        b.set_boxes(boxes, ALPHA)
        b.volume_trial_replicas(boxes * np.array([1.01, 0.0]))
        expect(_lib.MMC_ERR_STATE, b)
        expect(_lib.MMC_ERR_STATE, b, per=True)
        b.volume_settle(np.zeros(R, dtype=np.int32))
        assert flat(b.sdf(N_HALF, CELL, per_replica=True)).tobytes() == base.tobytes()
        for kw in (dict(cell=0.0), dict(cell=float("nan")), dict(fold=4), dict(site_mask=0), dict(site_mask=8),
                   dict(cell=0.7)):                                   # sqrt(3) 5.6 + rho > 10
            expect(_lib.MMC_ERR_ARG, b, **kw)
            expect(_lib.MMC_ERR_ARG, b, per=True, **kw)
        assert _lib.lib().mmc_batch_sdf(b._h, N_HALF, CELL, 3, 1, 0, None) == _lib.MMC_ERR_ARG
    with make_batch(a, R) as b:
        # proposals outstanding
        b.eval(np.full(R, 3), np.tile(a["com"][2], (R, 1)), np.tile(a["coords"][6:9], (R, 1, 1)))
        expect(_lib.MMC_ERR_STATE, b)
        expect(_lib.MMC_ERR_STATE, b, per=True)
        expect(_lib.MMC_ERR_ARG, b, site_mask=0)                  # arguments come before the state
        b.settle(np.zeros(R, dtype=np.int32))
        # ... and after moves of the caller's own the batch no longer vouches for the molecules' extent
        expect(_lib.MMC_ERR_ARG, b)
    with make_batch(a, R) as b:
        b.set_option("device_moves", 1)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        b.run(10, T, DR, DPHI, seed=3, energies=e)
        assert b.sdf(N_HALF, CELL).grid.sum() > 0                    # the device's own rigid moves keep the bound
