"""mmc_batch_voronoi against its numpy restatement (tests/voronoi_ref.py).

Everything is compared exactly: the five histograms, flagged, faces and nbr as integers; vol, area,
face_area and sums bit for bit (NaN where the restatement has NaN) -- every operation between the
coordinates and these values is a correctly rounded + - x / or sqrt in the header's order, with
nothing fused, and sums are added in k_local_qsum's fixed order.  What the frames cover is asserted
on the restatement by test_voronoi_host.py.

The restatement takes about 14 ms a molecule, so frames of hundreds of molecules are compared in
two parts: the per-molecule outputs of a subset of the molecules against the restatement of those
cells (a cell depends on nothing but its own list), and the histograms, flags and sums of every
replica against what the header's arithmetic makes of the call's own per-molecule outputs
(voronoi_ref.from_details).  side_hist does not follow from them and is compared in full on the
frames that are restated whole: every small frame, and configurations 3 and 4 as they stand (one
restatement each, kept by voronoi_ref.nist_cells and shared with the CPU tests).

Launch shape: k_voronoi_wave's unit is a molecule; workgroup g of G takes the molecules
[R N g / G, R N (g + 1) / G) of the replica-major order and its waves share the run's molecules of
one replica after the other.  G is option "wave_wgs"."""
import numpy as np
import pytest

import common
import voronoi_ref as ref
from metropolismontecarlo_amd import _lib, structs

pytestmark = pytest.mark.gpu

RCUT = 10.0
T, DR, DPHI = 298.15, 0.3, 0.2
ALPHA = 5.6
HISTS = ("vol_hist", "eta_hist", "face_hist", "side_hist", "nbr_hist")
BITS = ("vol", "area", "face_area")


def make_batch(a, R, rcut=RCUT):
    from metropolismontecarlo_amd.device import Batch
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
              ALPHA / a["box"], structs.factor, min(rcut, 0.5 * a["box"]), min(rcut, 0.5 * a["box"]))
    b.recip_long()
    return b


def same_bits(dev, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(dev), nan) and np.array_equal(dev[~nan].view(np.uint64), want[~nan].view(np.uint64))


def check_batch(b, boxes, p=None, replicas=None, mols=None, what="", cache=None):
    """One detailed per-replica call and one summed call: against the restatement of the replicas in
    `replicas` (default all; `mols`: of those molecules only; `cache`: a dict that keeps the
    restatements between calls on the same coordinates), every replica against its own
    per-molecule outputs, and the two calls against each other."""
    p = ref.params() if p is None else p
    R, N = b.R, b.n_mol
    per = b.voronoi(**p, per_replica=True, details=True)
    tot = b.voronoi(**p)
    shapes = dict(vol_hist=(p["v_bins"] + 1,), eta_hist=(p["eta_bins"] + 1,), face_hist=(65,), side_hist=(17,),
                  nbr_hist=(p["r_bins"] + 1,))
    for k, s in shapes.items():
        assert per[k].shape == (R,) + s and tot[k].shape == s and per[k].dtype == np.uint64
    assert per["flagged"].shape == (R, 3) and per["sums"].shape == (R, 8)
    assert per["vol"].shape == (R, N) and per["area"].shape == (R, N) and per["faces"].shape == (R, N)
    assert per["nbr"].shape == (R, N, 64) and per["face_area"].shape == (R, N, 64)
    for r in (range(R) if replicas is None else replicas):
        coords = b.get_replica(r)[1]
        key = (r, tuple(sorted(p.items())))
        want = cache.get(key) if cache is not None else None
        if want is None:
            want = ref.voronoi(coords, float(boxes[r]), **p, mols=mols)
            if cache is not None:
                cache[key] = want
        rows = slice(None) if mols is None else np.asarray(mols)
        assert np.array_equal(per["faces"][r][rows], want["faces"][rows]), (what, r)
        assert np.array_equal(per["nbr"][r][rows], want["nbr"][rows]), (what, r)
        for k in BITS:
            assert same_bits(per[k][r][rows], want[k][rows]), (what, r, k)
        if mols is None:
            for k in HISTS:
                assert np.array_equal(per[k][r], want[k]), (what, r, k)
            assert np.array_equal(per["flagged"][r], want["flagged"]), (what, r)
            assert same_bits(per["sums"][r], want["sums"]), (what, r, per["sums"][r] - want["sums"])
    for r in range(R):                                         # every replica: the outputs against each other
        own = ref.from_details(b.get_replica(r)[1], float(boxes[r]), per["vol"][r], per["area"][r], per["faces"][r],
                               per["nbr"][r], **p, face_area=per["face_area"][r])
        for k in ("vol_hist", "eta_hist", "face_hist", "nbr_hist", "flagged"):
            assert np.array_equal(per[k][r], own[k]), (what, r, k)
        assert same_bits(per["sums"][r], own["sums"]), (what, r, per["sums"][r] - own["sums"])
        ok = per["faces"][r] >= 0
        assert per["side_hist"][r].sum() == per["faces"][r][ok].sum() and not per["side_hist"][r][:3].any(), (what, r)
        assert np.array_equal(np.isnan(per["vol"][r]), ~ok) and np.array_equal(np.isnan(per["area"][r]), ~ok), (what, r)
        listed = np.where(ok, per["faces"][r], 0)[:, None] > np.arange(64)[None, :]
        assert np.array_equal(per["nbr"][r] >= 0, listed) and np.array_equal(per["face_area"][r] > 0.0, listed), (what, r)
        assert np.all(per["face_area"][r][listed] > p["area_min"]), (what, r)
    # summed outputs, and identical bits from call to call
    for k in HISTS:
        assert np.array_equal(tot[k], per[k].sum(0)), (what, k)
    assert np.array_equal(tot["flagged"], per["flagged"]), what
    assert np.array_equal(tot["sums"].view(np.uint64), per["sums"].view(np.uint64)), what
    again = b.voronoi(**p, per_replica=True, details=True)
    for k in per:
        assert np.array_equal(per[k].view(np.uint8), again[k].view(np.uint8)), (what, k)
    return per, tot


@pytest.mark.parametrize("n_mol", ref.SIZES)
def test_small_and_odd_systems(n_mol):
    """Two, three, one lane pass (64), a second pass with one and two molecules (65, 66), three
    passes (129) in a 22 A box: all or mostly OPEN, and at 129 and L / 2 lists that pass 64 entries
    inside the scan (CAP); mixed atom types, so the SoA arrays are read; three replicas that
    differ; bin counts 1, 7 and 1024."""
    a = ref.random_frame(n_mol)
    cases = {"7": ref.params(v_bins=7, eta_bins=7, r_bins=7),
             "L/2": ref.params(r_list=0.5 * ref.BOX, v_bins=1024, eta_bins=1024, r_bins=1024, v_max=400.0),
             "5": ref.params(r_list=5.0, v_bins=1, eta_bins=1, r_bins=1, area_min=0.01)}
    with make_batch(a, 3) as b:
        for r in (1, 2):
            b.set_replica(r, *ref.replica_frame(a, r))
        b.recip_long()
        flagged, cache = np.zeros(3, np.int64), {}
        for stage in (1, 0):                                   # staged in LDS; read from device memory
            b.set_option("local_stage", stage)
            for name, p in cases.items():
                per, _ = check_batch(b, [ref.BOX] * 3, p, what=f"n_mol {n_mol}, r_list {name}, stage {stage}",
                                     cache=cache)
                flagged += per["flagged"].sum(0).astype(np.int64)
        assert flagged[1] > 0 and flagged[2] == 0 and (flagged[0] > 0) == (n_mol == 129)


@pytest.mark.parametrize("n_mol", [65, 66])
def test_oxygens_in_a_ball_fill_the_list_exactly_or_flag_everything(n_mol):
    a = ref.ball_frame(n_mol)
    with make_batch(a, 2) as b:
        cache = {}
        for stage in (1, 0):
            b.set_option("local_stage", stage)
            per, tot = check_batch(b, [ref.BOX] * 2, what=f"ball {n_mol}, stage {stage}", cache=cache)
            if n_mol == 65:                                    # the inner cells of the cluster are closed
                assert not per["flagged"][:, 0].any() and np.all(per["flagged"][:, 1] > 0) and np.all(per["sums"][:, 0] > 0)
            else:
                assert np.all(per["flagged"] == [66, 0, 0]) and np.all(per["faces"] == -1) and np.all(per["nbr"] == -1)
                assert all(tot[k].sum() == 0 for k in HISTS) and np.all(np.isnan(per["vol"])) and np.all(per["sums"] == 0.0)


def test_the_simple_cubic_lattice_and_ties_to_the_lower_index():
    """Six neighbours at bit-equal r^2, twelve and eight more at two others: every cell a cube, the
    geometric neighbours the six nearest in index order, and more faces than six without area_min."""
    n, a_lat, basis, r_list, eta, faces, per_cell = ref.LATTICES["sc"]
    a, _ = ref.lattice("sc")
    with make_batch(a, 2) as b:
        p = ref.params(r_list=r_list, area_min=1e-6, v_max=200.0)
        per, _ = check_batch(b, [a["box"]] * 2, p, what="sc")
        assert not per["flagged"].any() and np.all(per["faces"] == 6) and per["side_hist"][0, 4] == 6 * n ** 3
        assert np.abs(per["vol"] / a_lat ** 3 - 1.0).max() < 1e-12
        assert abs(per["sums"][0, 1] / a["box"] ** 3 - 1.0) < 1e-12
        _, r2 = ref.oo_vectors(a["coords"], a["box"])
        for i in range(n ** 3):
            assert list(per["nbr"][0, i, :6]) == sorted(np.flatnonzero(r2[i] == a_lat * a_lat)), i
        b.set_option("local_stage", 0)
        raw, _ = check_batch(b, [a["box"]] * 2, ref.params(r_list=r_list, v_max=200.0), what="sc, area_min 0, unstaged")
        assert raw["faces"].max() > 6 and same_bits(raw["vol"], per["vol"])


def test_the_jittered_diamond_lattice():
    a, r_list = ref.lattice("diamond", 0.3)
    with make_batch(a, 2) as b:
        p = ref.params(r_list=r_list, area_min=1e-6, v_max=200.0)
        per, _ = check_batch(b, [a["box"]] * 2, p, what="diamond")
        assert not per["flagged"].any()
        assert abs(per["sums"][0, 1] / a["box"] ** 3 - 1.0) < 1e-12 and abs(per["vol"][0].sum() / a["box"] ** 3 - 1.0) < 1e-12
        assert per["side_hist"][0, 10:].sum() > 0              # the large polygons of the open structure


def test_coincident_oxygens_are_open():
    """rho = 0 has no bisector plane: both molecules of the pair are OPEN (the header) and the call
    returns.  A third molecule that lists both owns two faces in bit-equal planes; what becomes of
    them is what the header's arithmetic gives (either may vanish), and is compared as such."""
    a = ref.coincident_frame()
    with make_batch(a, 2) as b:
        per, _ = check_batch(b, [ref.BOX] * 2, ref.params(r_list=0.5 * ref.BOX), what="coincident")
        assert per["faces"][0, 0] == -2 and per["faces"][0, 1] == -2


@pytest.mark.parametrize("sides", [16, 17])
def test_a_ring_of_tangent_planes_reaches_maxv_and_passes_it(sides):
    """The restatement can build the POLY polygon: 16 tangent planes around one close pair leave
    two faces of MAXV = 16 sides and the cell whole, 17 flag it POLY."""
    a = ref.ring_frame(sides)
    with make_batch(a, 2) as b:
        per, _ = check_batch(b, [ref.BOX] * 2, ref.params(r_list=ref.RING_R_LIST), what=f"ring {sides}")
        if sides == 16:
            assert per["faces"][0, 0] == 18 and per["side_hist"][0, 16] == 2
        else:
            assert per["faces"][0, 0] == -4 and per["flagged"][0, 2] >= 1       # (the close pair sees the ring too)


def test_one_molecule_is_refused():
    a = ref.random_frame(1)
    with make_batch(a, 2) as b:
        out = sentinels(b, ref.params())
        with pytest.raises(_lib.MMCError) as ei:
            b.voronoi(details=True, out=out)
        assert ei.value.status == _lib.MMC_ERR_UNSUPPORTED and untouched(out)


def test_nist_config_1_is_mostly_open():
    """100 molecules in a 20 A box: r_list can be 10 A at most; most molecules have more than 64
    neighbours inside it or a cell that reaches beyond 5 A."""
    a = common.nist_arrays(1, "unwrapped")
    with make_batch(a, 3) as b:
        b.run(150, T, 0.4, 0.2, seed=2, n_groups=1)            # replicas diverge
        per, _ = check_batch(b, [a["box"]] * 3, ref.params(r_list=0.5 * a["box"], v_max=400.0), what="cfg1")
        assert np.all((per["faces"] < 0).sum(1) > 50) and np.all(per["flagged"][:, 1] > 0)
        assert not np.array_equal(per["faces"][0], per["faces"][1])


@pytest.mark.parametrize("variant", ["unwrapped", "reference"])
def test_nist_config_3_in_both_com_conventions(variant):
    """300 molecules at 1 g/cm^3 with r_list = 6: nothing is flagged (test_voronoi_host.py), so the
    cells fill the box."""
    a, want, _ = ref.nist_cells(3, variant, 6.0)
    with make_batch(a, 2) as b:
        p = ref.params(r_list=6.0)
        per, tot = check_batch(b, [a["box"]] * 2, p, replicas=[1], mols=range(0, 300, 6), what=variant)
        coords0 = b.get_replica(0)[1]
        if not np.array_equal(coords0, a["coords"]):           # (the restatement of the fixture is shared with the CPU tests)
            want = ref.voronoi(coords0, a["box"], **p)
        for k in ("faces", "nbr"):
            assert np.array_equal(per[k][0], want[k]), k
        for k in BITS:
            assert same_bits(per[k][0], want[k]), k
        for k in HISTS + ("flagged",):
            assert np.array_equal(per[k][0], want[k]), k
        assert same_bits(per["sums"][0], want["sums"])
        assert not per["flagged"].any()
        for r in range(2):
            assert abs(per["vol"][r].sum() / a["box"] ** 3 - 1.0) < 1e-12 and abs(per["sums"][r, 1] / a["box"] ** 3 - 1.0) < 1e-12
        from metropolismontecarlo_amd import observables as obs
        v, eta, faces = obs.voronoi_means(tot["sums"].sum(0))
        assert abs(v - a["box"] ** 3 / 300) < 1e-9 and 1.5 < eta < 1.9 and 14.0 < faces < 17.0
        assert obs.volume_fluctuation(tot["sums"].sum(0)) > 0.0
        n, pn, mean = obs.voronoi_coordination(tot["face_hist"])
        assert abs(mean - faces) < 1e-12 and abs(pn.sum() - 1.0) < 1e-12
        k, pk, sides = obs.face_side_fractions(tot["side_hist"])
        assert abs(sides - (6.0 - 12.0 / faces)) < 1e-9        # Euler: three faces meet at every vertex
        r, g = obs.voronoi_neighbour_gr(tot["nbr_hist"], 6.0, tot["sums"][:, 0].sum(), 300 / a["box"] ** 3)
        assert 2.0 < g.max() < 4.0 and 2.6 < r[np.argmax(g)] < 2.9   # the first peak of g_OO is all geometric neighbours
        vc, pv, beyond = obs.voronoi_volume_distribution(tot["vol_hist"], 80.0)
        ec, pe, _ = obs.asphericity_distribution(tot["eta_hist"], 3.0)
        assert beyond == 0.0 and abs((pv * vc).sum() * (vc[1] - vc[0]) - v) < 0.5 and abs((pe * ec).sum() * (ec[1] - ec[0]) - eta) < 0.02


def whole_replica(per, r, want, what, hists=HISTS):
    """Every output of replica r against a whole restatement (`hists`: those of them whose bins the
    restatement shares with the call)."""
    assert np.array_equal(per["faces"][r], want["faces"]) and np.array_equal(per["nbr"][r], want["nbr"]), what
    for k in BITS:
        assert same_bits(per[k][r], want[k]), (what, k)
    for k in hists + ("flagged",):
        assert np.array_equal(per[k][r], want[k]), (what, k)
    assert same_bits(per["sums"][r], want["sums"]), (what, per["sums"][r] - want["sums"])


def test_750_molecules():
    """The workload's own size (configuration 4, r_list 7.5): the fixture as it stands against its
    whole restatement (shared with test_voronoi_host.py, which pins it: every cell, side_hist
    included), then two replicas after a few dozen moves."""
    a, want, _ = ref.nist_cells(4, "unwrapped", 7.5)
    with make_batch(a, 2) as b:
        assert np.array_equal(b.get_replica(0)[1], a["coords"])
        first = b.voronoi(r_list=7.5, per_replica=True, details=True)
        for r in range(2):
            whole_replica(first, r, want, f"cfg4 as it stands, replica {r}")
        b.set_option("device_moves", 1)
        b.run(48, T, DR, DPHI, seed=4242)
        p = ref.params(r_list=7.5)
        per, tot = check_batch(b, [a["box"]] * 2, p, mols=range(3, 750, 11), what="cfg4")
        assert not per["flagged"][:, 0].any() and not per["flagged"][:, 2].any()
        assert np.all(per["flagged"][:, 1] > 0) and np.all(per["flagged"][:, 1] <= 0.05 * 750)
        assert not np.array_equal(per["faces"][0], per["faces"][1])
        b.set_option("voronoi_prune", 0)                       # every plane: the same bits
        full = b.voronoi(**p, per_replica=True, details=True)
        for k in per:
            assert np.array_equal(per[k].view(np.uint8), full[k].view(np.uint8)), k


def test_counters_that_leave_a_workgroup_fewer_waves():
    """The waves' lists and polygons (768 + 16384 bytes each), the workgroup's counters and the
    staged positions share the device's LDS less 64 bytes (160 KiB on the MI355X: 163776 bytes).
    750 molecules are 18000 bytes; three histograms of 1024 bins make 3 + 3 x 1025 + 65 + 17 = 3160
    counters, 12640 bytes: eight waves would need 137216 + 12640 + 18000 = 167856 bytes, seven need
    150704, so the staged launch has SEVEN waves (a stride that is no power of two); with the
    default bins (768 counters), and unstaged with either, it has eight.  Replica 0 is the fixture as
    it stands, compared whole; replica 1 is shifted.  All launch shapes give the same bits."""
    a, want, _ = ref.nist_cells(4, "unwrapped", 7.5)
    lds, big, small = 160 * 1024 - 64, 4 * 3160, 4 * 768
    assert 8 * 17152 + big + 24 * 750 > lds >= 7 * 17152 + big + 24 * 750 and 8 * 17152 + small + 24 * 750 <= lds
    p = ref.params(r_list=7.5, v_bins=1024, eta_bins=1024, r_bins=1024)
    with make_batch(a, 2) as b:
        sh = np.array([1.7, -2.9, 0.4])
        b.set_replica(1, a["com"] + sh, a["coords"] + sh)
        b.recip_long()
        assert np.array_equal(b.get_replica(0)[1], a["coords"])
        seven, seven_tot = check_batch(b, [a["box"]] * 2, p, replicas=[1], mols=range(5, 750, 25), what="seven waves")
        whole_replica(seven, 0, want, "seven waves", hists=("face_hist", "side_hist"))
        assert not np.array_equal(seven["vol"][0].view(np.uint64), seven["vol"][1].view(np.uint64))
        eight = b.voronoi(r_list=7.5, per_replica=True, details=True)      # default bins: eight waves, staged
        whole_replica(eight, 0, want, "eight waves")
        for k in BITS + ("faces", "nbr", "flagged", "sums", "face_hist", "side_hist"):
            assert np.array_equal(seven[k].view(np.uint8), eight[k].view(np.uint8)), k
        for wgs, stage in ((1, 1), (2, 1), (1, 0), (0, 0)):
            b.set_option("wave_wgs", wgs)
            b.set_option("local_stage", stage)
            per = b.voronoi(**p, per_replica=True, details=True)
            tot = b.voronoi(**p)
            for k in seven:
                assert np.array_equal(per[k].view(np.uint8), seven[k].view(np.uint8)), (wgs, stage, k)
            for k in seven_tot:
                assert np.array_equal(tot[k].view(np.uint8), seven_tot[k].view(np.uint8)), (wgs, stage, k)
        b.set_option("wave_wgs", 0)
        b.set_option("local_stage", 1)


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
        mols = range(1, 750, 15)
        per, _ = check_batch(b, boxes, ref.params(r_list=7.5), mols=mols, what="per box")
        assert np.all(per["sums"][:, 0] > 600) and per["flagged"][0, 1] < per["flagged"][2, 1]   # the wider box has larger cells
        e0 = b.potential_ewald(as_array=True)["energy"].copy()
        b.run_npt_replicas(2, T, 0.0024, 300.0, DR, DPHI, seed=9, energies=e0, moves_per_sweep=40)
        boxes = b.get_boxes()
        half = 0.5 * boxes.min()
        per, _ = check_batch(b, boxes, ref.params(r_list=half), mols=mols, what="per box, half the smallest box")
        assert per["flagged"][:, 0].sum() == per["faces"].size  # hundreds inside 14 A: nothing is truncated
        out = sentinels(b, ref.params())
        with pytest.raises(_lib.MMCError) as ei:
            b.voronoi(r_list=np.nextafter(half, 100.0), details=True, out=out)
        assert ei.value.status == _lib.MMC_ERR_ARG and untouched(out)


@pytest.mark.parametrize("system", ["records", "arrays"])
def test_launch_shape_does_not_change_the_results(system):
    """One and two workgroups, the default grid, staged and unstaged, with every replica's cells
    against a few restated ones; with records, 2.5 replicas per workgroup of the default grid."""
    n_cus = common.device_cu_count()
    R = (5 * n_cus) // 2 + 1
    a = common.nist_arrays(1, "unwrapped") if system == "records" else ref.random_frame(65, seed=17)
    p = ref.params(r_list=7.0, v_bins=64, eta_bins=50, v_max=300.0)
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
        base_per = b.voronoi(**p, per_replica=True, details=True)
        base_tot = b.voronoi(**p)
        for r in sorted({0, 1, R // 2, R - 1}):
            want = ref.voronoi(b.get_replica(r)[1], a["box"], **p)
            for k in HISTS + ("flagged", "faces", "nbr"):
                assert np.array_equal(base_per[k][r], want[k]), (system, r, k)
            for k in BITS + ("sums",):
                assert same_bits(base_per[k][r], want[k]), (system, r, k)
        assert (base_per["sums"][:, 0].sum() > 0) == (system == "records")   # the sparse random frame: every cell open
        for wgs, stage in ((1, 1), (2, 1), (3, 0), (0, 0), (1, 0)):
            b.set_option("wave_wgs", wgs)
            b.set_option("local_stage", stage)
            per = b.voronoi(**p, per_replica=True, details=True)
            tot = b.voronoi(**p)
            for k in base_per:
                assert np.array_equal(per[k].view(np.uint8), base_per[k].view(np.uint8)), (system, wgs, stage, k)
            for k in base_tot:
                assert np.array_equal(tot[k].view(np.uint8), base_tot[k].view(np.uint8)), (system, wgs, stage, k)
        b.set_option("wave_wgs", 0)
        b.set_option("local_stage", 1)


OUTPUTS = HISTS + ("flagged", "sums", "vol", "area", "faces", "nbr", "face_area")
CT = {np.dtype(np.uint64): _lib.C.c_uint64, np.dtype(np.float64): _lib.C.c_double, np.dtype(np.int32): _lib.C.c_int32}


def test_null_outputs_cost_nothing_and_change_nothing():
    """Each output alone, each left out alone, and a few mixed sets, through the C call: the same
    numbers as all together, and an array that is not passed is not written."""
    a = common.nist_arrays(1, "unwrapped")
    with make_batch(a, 2) as b:
        p = ref.params(r_list=8.0)
        full = b.voronoi(**p, details=True)
        L = _lib.lib()
        sets = [{k} for k in OUTPUTS] + [set(OUTPUTS) - {k} for k in OUTPUTS]
        sets += [{"flagged", "nbr"}, {"sums", "face_area"}, {"side_hist", "faces"}, {"vol", "nbr_hist", "eta_hist"}]
        for chosen in sets:
            got = {k: np.full_like(full[k], 99) for k in OUTPUTS}
            ptrs = [got[k].ctypes.data_as(_lib.C.POINTER(CT[got[k].dtype])) if k in chosen else None for k in OUTPUTS]
            st = L.mmc_batch_voronoi(b._h, p["r_list"], p["area_min"], p["v_bins"], p["v_max"], p["eta_bins"], p["eta_max"],
                                     p["r_bins"], 0, *ptrs)
            assert st == _lib.MMC_OK, chosen
            for k in OUTPUTS:
                if k in chosen:
                    assert np.array_equal(got[k].view(np.uint8), full[k].view(np.uint8)), (chosen, k)
                else:
                    assert np.all(got[k] == 99), (chosen, k)


def chain(b, interleave, n_blocks=2, steps=60):
    e = b.potential_ewald(as_array=True)["energy"].copy()
    stats = []
    for blk in range(n_blocks):
        e, st = b.run(steps, T, DR, DPHI, seed=21, energies=e)
        stats.append({k: v for k, v in st.items() if isinstance(v, int)})
        if interleave:
            b.voronoi(r_list=7.5, per_replica=bool(blk & 1), details=bool(blk & 1))
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
    a = common.nist_arrays(3, "unwrapped")
    with make_batch(a, 2, rcut=9.0) as b:
        b.set_option("device_moves", 1)
        b.set_coulomb_style("wolf")
        e = b.potential_wolf(as_array=True)["energy"].copy()
        b.run(90, T, 0.4, 0.2, seed=8, energies=e)
        per, _ = check_batch(b, [a["box"]] * 2, ref.params(r_list=6.0), mols=range(2, 300, 10), what="wolf")
        assert not np.array_equal(per["vol"][0].view(np.uint64), per["vol"][1].view(np.uint64))


def sentinels(b, p, per_replica=False):
    R, N = b.R, b.n_mol
    lead = (R,) if per_replica else ()
    nv, ne, nr = (max(int(p[k]), 0) for k in ("v_bins", "eta_bins", "r_bins"))
    return dict(vol_hist=np.full(lead + (nv + 1,), 99, dtype=np.uint64), eta_hist=np.full(lead + (ne + 1,), 99, dtype=np.uint64),
                face_hist=np.full(lead + (65,), 99, dtype=np.uint64), side_hist=np.full(lead + (17,), 99, dtype=np.uint64),
                nbr_hist=np.full(lead + (nr + 1,), 99, dtype=np.uint64), flagged=np.full((R, 3), 99, dtype=np.uint64),
                sums=np.full((R, 8), 7.5), vol=np.full((R, N), 7.5), area=np.full((R, N), 7.5),
                faces=np.full((R, N), -5, dtype=np.int32), nbr=np.full((R, N, 64), -5, dtype=np.int32),
                face_area=np.full((R, N, 64), 7.5))


def untouched(out):
    return (all(np.all(out[k] == 99) for k in HISTS + ("flagged",)) and all(np.all(out[k] == 7.5) for k in ("sums",) + BITS)
            and np.all(out["faces"] == -5) and np.all(out["nbr"] == -5))


def test_refusals_leave_outputs_untouched():
    a = common.nist_arrays(1, "unwrapped")
    R = 2

    def expect(status, b, per=False, **kw):
        p = ref.params(**kw)
        out = sentinels(b, p, per)
        with pytest.raises(_lib.MMCError) as ei:
            b.voronoi(**p, per_replica=per, details=True, out=out)
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
        for kw in (dict(area_min=-1.0), dict(area_min=float("nan")), dict(v_bins=0), dict(v_bins=1025), dict(v_max=0.0),
                   dict(v_max=float("inf")), dict(eta_bins=0), dict(eta_bins=1025), dict(eta_max=1.0),
                   dict(eta_max=float("nan")), dict(r_bins=0), dict(r_bins=1025)):
            expect(_lib.MMC_ERR_ARG, b, **kw)
        # ... and after all that the call works: the largest bins and r_list = L / 2 exactly
        res = b.voronoi(r_list=a["box"] / 2, v_bins=1024, eta_bins=1024, r_bins=1024)
        assert res["vol_hist"].sum() == res["sums"][:, 0].sum() == R * b.n_mol - res["flagged"][:, :2].sum()
    # a volume trial in flight
    with per_box_batch(per_box_states([1.0, 1.02])) as b:
        boxes = b.get_boxes()
        b.volume_trial_replicas(boxes * np.array([1.01, 0.0]))
        expect(_lib.MMC_ERR_STATE, b)
        b.volume_settle(np.zeros(R, dtype=np.int32))
        res = b.voronoi()
        assert res["face_hist"].sum() == res["sums"][:, 0].sum() == R * b.n_mol - res["flagged"][:, 1].sum()
