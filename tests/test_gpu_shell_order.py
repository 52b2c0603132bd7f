"""mmc_batch_shell_order against its numpy restatement (tests/shell_order_ref.py).

Everything is compared exactly: the four histograms, flagged, count and nbr as integers, lsi and zeta
bit for bit (NaN where the restatement has NaN) -- every operation between the coordinates and these
values is a correctly rounded + - x / or sqrt in the header's order, with nothing fused.  sums[r] is
within 1e-12 N of the sums of the device's own lsi and zeta, exact in its counts, and bit-identical
between calls.  What the frames cover is asserted on the restatement by test_shell_order_host.py.

Launch shape: k_shell_order_wave's unit is a molecule; workgroup g of G takes the molecules
[R N g / G, R N (g + 1) / G) of the replica-major order and its waves share the run's molecules of
one replica after the other.  G is option "wave_wgs"; with wave_wgs = 1 the waves of one workgroup
walk every replica, and with R > 2.5 x 4 x n_cus the default grid gives every wave molecules of two
or three replicas."""
import numpy as np
import pytest

import common
import shell_order_ref as ref
from metropolismontecarlo_amd import _lib, structs

pytestmark = pytest.mark.gpu

RCUT = 10.0
T, DR, DPHI = 298.15, 0.3, 0.2
ALPHA = 5.6
HISTS = ("rank_hist", "lsi_hist", "ang_hist", "zeta_hist")


def make_batch(a, R, rcut=RCUT):
    from metropolismontecarlo_amd.device import Batch
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
              ALPHA / a["box"], structs.factor, rcut, rcut)
    b.recip_long()
    return b


def same_bits(dev, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(dev), nan) and np.array_equal(dev[~nan].view(np.uint64), want[~nan].view(np.uint64))


def check_batch(b, boxes, p=None, replicas=None, what=""):
    """One detailed per-replica call and one summed call against the restatement of every replica
    in `replicas` (default all) and against each other."""
    p = ref.params() if p is None else p
    R, N = b.R, b.n_mol
    per = b.shell_order(**p, per_replica=True, details=True)
    tot = b.shell_order(**p)
    shapes = dict(rank_hist=(p["n_rank"], p["r_bins"] + 1), lsi_hist=(p["lsi_bins"] + 1,),
                  ang_hist=(p["ang_bins"] + 1,), zeta_hist=(p["zeta_bins"] + 1,))
    for k, s in shapes.items():
        assert per[k].shape == (R,) + s and tot[k].shape == s and per[k].dtype == np.uint64
    assert per["flagged"].shape == (R,) and per["sums"].shape == (R, 4)
    assert per["count"].shape == (R, N) and per["nbr"].shape == (R, N, 16)
    assert per["lsi"].shape == (R, N) and per["zeta"].shape == (R, N)
    for r in (range(R) if replicas is None else replicas):
        want = ref.shell_order(b.get_replica(r)[1], float(boxes[r]), **p)
        assert per["flagged"][r] == want["flagged"], (what, r)
        assert np.array_equal(per["count"][r], want["count"]), (what, r)
        assert np.array_equal(per["nbr"][r], want["nbr"]), (what, r)
        for k in HISTS:
            assert np.array_equal(per[k][r], want[k]), (what, r, k)
        assert same_bits(per["lsi"][r], want["lsi"]), (what, r, np.nanmax(np.abs(per["lsi"][r] - want["lsi"])))
        assert same_bits(per["zeta"][r], want["zeta"]), (what, r, np.nanmax(np.abs(per["zeta"][r] - want["zeta"])))
        ma = want["m_ang"][want["m_ang"] >= 0]
        assert per["ang_hist"][r].sum() == (ma * (ma - 1) // 2).sum(), (what, r)
    for r in range(R):                                         # every replica: the outputs against each other
        fl = int(per["flagged"][r])
        assert fl == np.count_nonzero(per["count"][r] < 0), (what, r)
        assert np.all(per["rank_hist"][r].sum(1) + fl == N), (what, r)
        assert per["lsi_hist"][r].sum() + fl == N and per["zeta_hist"][r].sum() + fl == N, (what, r)
        lsi, zeta = per["lsi"][r], per["zeta"][r]
        assert np.array_equal(np.bincount(ref.lsi_bin(lsi, p["lsi_bins"], p["lsi_max"])[per["count"][r] >= 0],
                                          minlength=p["lsi_bins"] + 1), per["lsi_hist"][r]), (what, r)
        assert np.array_equal(np.bincount(ref.zeta_bin(zeta, p["zeta_bins"], p["zeta_lo"], p["zeta_hi"])[per["count"][r] >= 0],
                                          minlength=p["zeta_bins"] + 1), per["zeta_hist"][r]), (what, r)
        fl_, fz_ = np.isfinite(lsi), np.isfinite(zeta)
        assert per["sums"][r, 1] == fl_.sum() and per["sums"][r, 3] == fz_.sum(), (what, r)
        assert abs(per["sums"][r, 0] - lsi[fl_].sum()) <= 1e-12 * N, (what, r)
        assert abs(per["sums"][r, 2] - zeta[fz_].sum()) <= 1e-12 * N, (what, r)
        listed = per["count"][r][:, None] > np.arange(16)[None, :]
        assert np.array_equal(per["nbr"][r] >= 0, listed), (what, r)
    # summed outputs, and identical bits from call to call
    for k in HISTS:
        assert np.array_equal(tot[k], per[k].sum(0)), (what, k)
    assert np.array_equal(tot["flagged"], per["flagged"]), what
    assert np.array_equal(tot["sums"].view(np.uint64), per["sums"].view(np.uint64)), what
    again = b.shell_order(**p, per_replica=True, details=True)
    for k in per:
        assert np.array_equal(per[k].view(np.uint8), again[k].view(np.uint8)), (what, k)
    return per, tot


@pytest.mark.parametrize("n_mol", ref.SIZES)
def test_small_and_odd_systems(n_mol):
    """The minimum of two, three, one lane pass (64), a second pass with one and two molecules (65,
    66), three passes (129); mixed atom types, so the SoA arrays are read; three replicas that
    differ.  r_list = 3.7, 7 and L / 2 with bin counts 1024, 7 and 1 and n_rank 1 and 16: at 129 molecules and L / 2 most lists pass 64 entries inside the scan and some
    stop at exactly 64."""
    a = ref.random_frame(n_mol)
    with make_batch(a, 3) as b:
        for r in (1, 2):
            b.set_replica(r, *ref.replica_frame(a, r))
        b.recip_long()
        flagged = 0
        for stage in (1, 0):                                   # staged in LDS; read from device memory
            b.set_option("local_stage", stage)
            for name, p in ref.CASES.items():
                per, _ = check_batch(b, [ref.BOX] * 3, p, what=f"n_mol {n_mol}, r_list {name}, stage {stage}")
                flagged += int(per["flagged"].sum())
        assert (flagged > 0) == (n_mol == 129)


@pytest.mark.parametrize("waves", [2, 1])
def test_counters_that_leave_a_workgroup_fewer_waves(waves):
    """The workgroup's counters and its waves' lists share 32 KiB: 7472 words leave two waves, 8000
    (the bound) one.  With one workgroup, so that its waves share every replica."""
    a = ref.random_frame(129)
    with make_batch(a, 3) as b:
        for r in (1, 2):
            b.set_replica(r, *ref.replica_frame(a, r))
        b.recip_long()
        check_batch(b, [ref.BOX] * 3, ref.FEWER_WAVES[waves], what=f"{waves} waves")
        b.set_option("wave_wgs", 1)
        b.set_option("local_stage", 0)
        check_batch(b, [ref.BOX] * 3, ref.FEWER_WAVES[waves], what=f"{waves} waves, one workgroup, unstaged")


@pytest.mark.parametrize("n_mol", [65, 66])
def test_oxygens_in_a_ball_fill_the_list_exactly_or_flag_everything(n_mol):
    a = ref.ball_frame(n_mol)
    with make_batch(a, 2) as b:
        for stage in (1, 0):
            b.set_option("local_stage", stage)
            per, tot = check_batch(b, [ref.BOX] * 2, what=f"ball {n_mol}, stage {stage}")
            if n_mol == 65:
                assert np.all(per["count"] == 64) and not per["flagged"].any()
            else:
                assert np.all(per["flagged"] == 66) and np.all(per["count"] == -1) and np.all(per["nbr"] == -1)
                assert all(tot[k].sum() == 0 for k in HISTS) and np.all(np.isnan(per["lsi"])) and np.all(per["sums"] == 0.0)


@pytest.mark.parametrize("n,spacing", [(4, 5.5), (5, 4.5)])
def test_lattice_ties_go_to_the_lower_index(n, spacing):
    """Six neighbours at bit-equal r^2 and twelve more at another: ranks among equal keys follow j."""
    a = ref.lattice_frame(n, spacing)
    p = ref.lattice_params(spacing)
    with make_batch(a, 2) as b:
        per, _ = check_batch(b, [a["box"]] * 2, p, what=f"lattice {n}")
        _, r2 = ref.oo_vectors(a["coords"], a["box"])
        for i in range(n ** 3):
            assert list(per["nbr"][0, i, :6]) == sorted(np.flatnonzero(r2[i] == spacing * spacing)), i
        assert np.all(per["count"] == 18) and per["ang_hist"][0, 0] == 3 * n ** 3
        b.set_option("local_stage", 0)
        check_batch(b, [a["box"]] * 2, p, what=f"lattice {n}, unstaged")


def test_coincident_oxygens_and_the_pentamer():
    a = ref.coincident_frame()
    with make_batch(a, 2) as b:
        per, _ = check_batch(b, [ref.BOX] * 2, ref.params(r_list=7.0, r_ang=7.0), what="coincident")
        assert per["ang_hist"][0, -1] > 0 and per["nbr"][0, 0, 0] == 1 and per["nbr"][0, 1, 0] == 0
    a = ref.pentamer_frame()
    with make_batch(a, 2) as b:
        per, _ = check_batch(b, [ref.BOX] * 2, what="pentamer")
        assert abs(per["zeta"][0, 0] - (ref.PENTAMER_FAR - ref.PENTAMER_R)) < 1e-12


def test_one_molecule_is_refused():
    a = ref.random_frame(1)
    with make_batch(a, 2) as b:
        out = sentinels(b, ref.params())
        with pytest.raises(_lib.MMCError) as ei:
            b.shell_order(details=True, out=out)
        assert ei.value.status == _lib.MMC_ERR_UNSUPPORTED and untouched(out)


@pytest.mark.parametrize("variant", ["unwrapped", "reference"])
def test_nist_config_1_in_both_com_conventions(variant):
    a = common.nist_arrays(1, variant)
    with make_batch(a, 3) as b:
        b.run(150, T, 0.4, 0.2, seed=2, n_groups=1)            # replicas diverge
        per, tot = check_batch(b, [a["box"]] * 3, what=variant)
        assert not np.array_equal(per["nbr"][0], per["nbr"][1])
        assert np.isfinite(per["lsi"]).sum() > 200 and np.isfinite(per["zeta"]).sum() > 200   # water: both are there
        b.set_option("local_stage", 0)
        check_batch(b, [a["box"]] * 3, ref.params(r_list=10.0, n_rank=16, r_bins=100), what=variant + ", unstaged")


def test_750_molecules():
    a = common.nist_arrays(4, "unwrapped")
    with make_batch(a, 3) as b:
        b.set_option("device_moves", 1)
        b.run(300, T, DR, DPHI, seed=4242)
        per, tot = check_batch(b, [a["box"]] * 3, what="cfg4")
        from metropolismontecarlo_amd import observables as obs
        assert per["flagged"].sum() == 0
        r, pk, beyond = obs.neighbour_distance_distributions(tot["rank_hist"], 6.0)
        d5 = (pk[4] * r).sum() * (r[1] - r[0])
        assert 3.0 < d5 < 4.5 and beyond[0] == 0.0              # water at 0.83 g/cm^3
        assert 0.0 < obs.lsi_mean(tot["sums"].sum(0)) < 0.3 and -1.0 < obs.zeta_mean(tot["sums"].sum(0)) < 1.5


def per_box_states(factors):
    a = common.nist_arrays(4, "unwrapped")
    out = []
    for f in factors:
        com = a["com"] * f
        out.append(dict(a, com=com, coords=a["coords"] + np.repeat(com - a["com"], 3, axis=0),
                        box=float(a["box"] * f)))
    return out


def per_box_batch(states):
    from metropolismontecarlo_amd.device import Batch
    a0 = states[0]
    b = Batch(len(states), a0["com"], a0["coords"], a0["atype"], a0["charge"], a0["eps"], a0["sig"],
              a0["box"], ALPHA / a0["box"], structs.factor, RCUT, RCUT)
    for r, a in enumerate(states):
        b.set_replica(r, a["com"], a["coords"])
    b.set_boxes([a["box"] for a in states], ALPHA)
    b.recip_long()
    return b


def test_per_replica_boxes():
    states = per_box_states([0.97, 1.0, 1.04])
    with per_box_batch(states) as b:
        boxes = b.get_boxes()
        check_batch(b, boxes, what="per box")
        e0 = b.potential_ewald(as_array=True)["energy"].copy()
        b.run_npt_replicas(2, T, 0.0024, 300.0, DR, DPHI, seed=9, energies=e0, moves_per_sweep=40)
        boxes = b.get_boxes()
        half = 0.5 * boxes.min()
        per, _ = check_batch(b, boxes, ref.params(r_list=half, r_bins=50), what="per box, half the smallest box")
        assert per["flagged"].sum() == per["count"].size       # hundreds inside 14 A: nothing is truncated
        per, _ = check_batch(b, boxes, ref.params(r_list=8.0, r_bins=50), replicas=[2], what="per box, 8 A")
        assert 0 < per["flagged"].sum() < per["count"].size
        out = sentinels(b, ref.params())
        with pytest.raises(_lib.MMCError) as ei:
            b.shell_order(r_list=np.nextafter(half, 100.0), details=True, out=out)
        assert ei.value.status == _lib.MMC_ERR_ARG and untouched(out)


@pytest.mark.parametrize("system", ["records", "arrays"])
def test_launch_shape_does_not_change_the_results(system):
    n_cus = common.device_cu_count()
    R = 10 * n_cus + 1                                      # 2.5 replicas per workgroup of the default grid
    a = common.nist_arrays(1, "unwrapped") if system == "records" else ref.random_frame(65, seed=17)
    p = ref.params(r_list=7.0, r_bins=64, lsi_bins=50)
    with make_batch(a, R) as b:
        if system == "records":
            b.set_option("device_moves", 1)
            b.run(30, T, 0.4, 0.2, seed=11)
        else:
            rng = np.random.default_rng(5)
            for r in range(1, R, max(1, R // 40)):             # some replicas moved as a whole
                sh = rng.random(3) * a["box"]
                b.set_replica(r, a["com"] + sh, a["coords"] + sh)
            b.recip_long()
        boxes = [a["box"]] * R
        some = sorted({0, 1, R // 2, R - 1})
        base_per, base_tot = check_batch(b, boxes, p, replicas=some, what=system)
        if system == "records":
            assert not np.array_equal(base_per["nbr"][0], base_per["nbr"][R - 1])
        for wgs, stage in ((1, 1), (3, 1), (0, 0), (1, 0)):
            b.set_option("wave_wgs", wgs)
            b.set_option("local_stage", stage)
            per = b.shell_order(**p, per_replica=True, details=True)
            tot = b.shell_order(**p)
            for k in base_per:
                assert np.array_equal(per[k].view(np.uint8), base_per[k].view(np.uint8)), (system, wgs, stage, k)
            for k in base_tot:
                assert np.array_equal(tot[k].view(np.uint8), base_tot[k].view(np.uint8)), (system, wgs, stage, k)
        b.set_option("wave_wgs", 0)
        b.set_option("local_stage", 1)


def test_null_outputs_cost_nothing_and_change_nothing():
    """Each histogram alone, and the sums alone, through the C call: the same numbers as together."""
    a = common.nist_arrays(1, "unwrapped")
    with make_batch(a, 2) as b:
        p = ref.params()
        full = b.shell_order(**p)
        L, u64 = _lib.lib(), _lib.C.POINTER(_lib.C.c_uint64)
        for pos, k in enumerate(HISTS + ("sums",)):
            got = np.zeros_like(full[k])
            ptrs = [None] * 5
            ptrs[pos] = got.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double) if k == "sums" else u64)
            st = L.mmc_batch_shell_order(b._h, p["r_list"], p["r_lsi"], p["r_ang"], p["r_hb"],
                                         float(np.cos(np.deg2rad(p["theta_deg"]))), p["n_rank"], p["r_bins"], p["lsi_bins"],
                                         p["lsi_max"], p["ang_bins"], p["zeta_bins"], p["zeta_lo"], p["zeta_hi"], 0,
                                         *ptrs[:4], None, ptrs[4], None, None, None, None)
            assert st == _lib.MMC_OK and np.array_equal(got.view(np.uint64), full[k].view(np.uint64)), k


def chain(b, interleave, n_blocks=2, steps=60):
    e = b.potential_ewald(as_array=True)["energy"].copy()
    stats = []
    for blk in range(n_blocks):
        e, st = b.run(steps, T, DR, DPHI, seed=21, energies=e)
        stats.append({k: v for k, v in st.items() if isinstance(v, int)})
        if interleave:
            b.shell_order(per_replica=bool(blk & 1), details=bool(blk & 1))
    return e, stats, [b.get_replica(r) for r in range(b.R)], b.potential_ewald(as_array=True)["energy"].copy()


def test_calls_between_blocks_leave_the_chain_bit_identical():
    """Coordinates, S(k) (get_replica's third array), energies and potential_ewald of 2 x 60 steps with
    a call after each block, against the same chain without."""
    a = common.nist_arrays(4, "unwrapped")
    runs = []
    for interleave in (False, True):
        with make_batch(a, 6) as b:
            b.set_option("device_moves", 1)
            runs.append(chain(b, interleave))
    x, y = runs
    assert np.array_equal(x[0].view(np.uint64), y[0].view(np.uint64))
    assert np.array_equal(x[3].view(np.uint64), y[3].view(np.uint64))
    assert x[1] == y[1]
    for p, q in zip(x[2], y[2]):
        assert all(np.array_equal(u.view(np.uint8), v.view(np.uint8)) for u, v in zip(p, q))


def test_wolf_style():
    a = common.nist_arrays(1, "unwrapped")
    with make_batch(a, 3) as b:
        b.set_option("device_moves", 1)
        b.set_coulomb_style("wolf")
        e = b.potential_wolf(as_array=True)["energy"].copy()
        b.run(90, T, 0.4, 0.2, seed=8, energies=e)
        per, _ = check_batch(b, [a["box"]] * 3, what="wolf")
        assert not np.array_equal(per["lsi"][0].view(np.uint64), per["lsi"][1].view(np.uint64))


def sentinels(b, p, per_replica=False):
    R, N = b.R, b.n_mol
    lead = (R,) if per_replica else ()
    nk, nr, nl, na, nz = (max(int(p[k]), 0) for k in ("n_rank", "r_bins", "lsi_bins", "ang_bins", "zeta_bins"))
    return dict(rank_hist=np.full(lead + (nk, nr + 1), 99, dtype=np.uint64), lsi_hist=np.full(lead + (nl + 1,), 99, dtype=np.uint64),
                ang_hist=np.full(lead + (na + 1,), 99, dtype=np.uint64), zeta_hist=np.full(lead + (nz + 1,), 99, dtype=np.uint64),
                flagged=np.full((R,), 99, dtype=np.uint64), sums=np.full((R, 4), 7.5),
                count=np.full((R, N), -5, dtype=np.int32), nbr=np.full((R, N, 16), -5, dtype=np.int32),
                lsi=np.full((R, N), 7.5), zeta=np.full((R, N), 7.5))


def untouched(out):
    return (all(np.all(out[k] == 99) for k in HISTS + ("flagged",)) and np.all(out["sums"] == 7.5)
            and np.all(out["count"] == -5) and np.all(out["nbr"] == -5) and np.all(out["lsi"] == 7.5)
            and np.all(out["zeta"] == 7.5))


def test_refusals_leave_outputs_untouched():
    a = common.nist_arrays(1, "unwrapped")
    R = 2

    def expect(status, b, per=False, **kw):
        p = ref.params(**kw)
        out = sentinels(b, p, per)
        with pytest.raises(_lib.MMCError) as ei:
            b.shell_order(**p, per_replica=per, details=True, out=out)
        assert ei.value.status == status and untouched(out), kw

    with make_batch(a, R) as b:
        # proposals outstanding
        com, coords = np.asarray(a["com"]), np.asarray(a["coords"])
        b.eval(np.full(R, 3), np.tile(com[2], (R, 1)), np.tile(coords[6:9], (R, 1, 1)))
        expect(_lib.MMC_ERR_STATE, b)
        expect(_lib.MMC_ERR_STATE, b, per=True)
        b.settle(np.zeros(R, dtype=np.int32))
        # bad arguments
        for r_list in (float("nan"), float("inf"), 0.0, -6.0, np.nextafter(a["box"] / 2, 100.0)):
            expect(_lib.MMC_ERR_ARG, b, r_list=r_list)
            expect(_lib.MMC_ERR_ARG, b, r_list=r_list, per=True)
        for kw in (dict(r_lsi=6.5), dict(r_ang=0.0), dict(r_hb=float("nan")), dict(theta_deg=120.0), dict(n_rank=0),
                   dict(n_rank=17), dict(r_bins=0), dict(r_bins=1025), dict(lsi_bins=1025), dict(lsi_max=0.0),
                   dict(ang_bins=0), dict(zeta_bins=1025), dict(zeta_lo=2.5), dict(zeta_hi=float("inf"))):
            expect(_lib.MMC_ERR_ARG, b, **kw)
        # the counters of one wave beyond the LDS bound: 16 x 1025 of the ranks alone, and one word too many
        expect(_lib.MMC_ERR_ARG, b, n_rank=16, r_bins=1024)
        expect(_lib.MMC_ERR_ARG, b, n_rank=7, r_bins=1023, lsi_bins=277, ang_bins=276, zeta_bins=276)
        # ... and after all that the call works: the bound itself, r_list = L / 2 and cos_hb = 1 exactly
        res = b.shell_order(r_list=a["box"] / 2, r_lsi=a["box"] / 2, theta_deg=0.0, n_rank=7, r_bins=1023, lsi_bins=276,
                            ang_bins=276, zeta_bins=276)
        assert np.all(res["rank_hist"].sum(1) + res["flagged"].sum() == R * b.n_mol)
    # a volume trial in flight
    with per_box_batch(per_box_states([1.0, 1.02])) as b:
        boxes = b.get_boxes()
        b.volume_trial_replicas(boxes * np.array([1.01, 0.0]))
        expect(_lib.MMC_ERR_STATE, b)
        b.volume_settle(np.zeros(R, dtype=np.int32))
        res = b.shell_order()
        assert res["lsi_hist"].sum() + res["flagged"].sum() == R * b.n_mol
