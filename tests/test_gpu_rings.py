"""mmc_batch_hbond_rings against its numpy restatement (tests/rings_ref.py).

Every output is an integer and must be equal exactly: the three rows of rings by size, the molecules
by membership, the eight sums and the counts per molecule, per replica and summed, from call to call
and whatever the launch shape.  The rows of `ring` are compared as a sorted set, with max_rings at
least the restatement's count, so that stats[6] == 0 is a condition of every comparison.

Launch shape: a replica is a workgroup's unit; workgroup g of G takes the replicas g, g + G, ...  G is
option "wave_wgs", by default what is resident; with details the replicas are worked off in launches
of option "ring_chunk" replicas."""
import numpy as np
import pytest

import common
import network_ref as net
import rings_ref as ref
from metropolismontecarlo_amd import _lib, structs
from test_gpu_network import (DPHI, DR, RCUT, T, make_batch, per_box_batch, per_box_states, shifted_replicas,
                              small_system)

pytestmark = pytest.mark.gpu

KEYS = ("ring_hist", "member_hist", "stats", "count")


def cosd(theta):
    return float(np.cos(np.deg2rad(float(theta))))


def sorted_rows(ring):
    return sorted(tuple(int(x) for x in row if x >= 0) for row in ring if row[0] >= 0)


def check_batch(b, boxes, r_hb=3.5, theta=30.0, n_max=8, replicas=None, what=""):
    """One detailed per-replica call and one summed call against the restatement of every replica in
    `replicas` (default all), against each other and against the identities between the outputs."""
    R, N = b.R, b.n_mol
    rs = list(range(R)) if replicas is None else list(replicas)
    wants = {r: ref.rings(b.get_replica(r)[1], float(boxes[r]), r_hb, cosd(theta), n_max) for r in rs}
    most = max(len(w["rows"]) for w in wants.values())
    max_rings = most + 1 if replicas is None else 2 * most + 64
    per = b.hbond_rings(r_hb, theta, n_max, per_replica=True, details=True, max_rings=max_rings)
    tot = b.hbond_rings(r_hb, theta, n_max)
    assert per["ring_hist"].shape == (R, 3, 9) and per["member_hist"].shape == (R, 9, 33) and per["stats"].shape == (R, 8)
    assert per["count"].shape == (R, N, 9) and per["ring"].shape == (R, max_rings, 8)
    assert tot["ring_hist"].shape == (3, 9) and tot["member_hist"].shape == (9, 33) and sorted(tot) == sorted(KEYS[:3])
    for r, want in wants.items():
        for key in KEYS:
            assert np.array_equal(per[key][r], want[key]), (what, r, key, per["stats"][r], want["stats"])
        assert per["stats"][r, 6] == 0 and sorted_rows(per["ring"][r]) == want["rows"], (what, r)
    for r in (range(R) if replicas is None else rs):           # the identities between the device's own outputs
        st, rh, mh, cnt, ring = (per[k][r] for k in ("stats", "ring_hist", "member_hist", "count", "ring"))
        if st[7]:
            assert list(st[:7]) == [0] * 7 and rh.sum() == 0 and mh.sum() == 0, (what, r)
            assert np.all(cnt == 65535) and np.all(ring == -1), (what, r)
            continue
        sizes = np.arange(9, dtype=np.uint64)
        assert rh[:, :3].sum() == 0 and rh[:, n_max + 1:].sum() == 0 and np.all(rh[2] <= rh[0]), (what, r)
        assert [rh[0].sum(), rh[1].sum(), rh[2].sum()] == list(st[1:4]), (what, r)
        assert (rh[0] * sizes).sum() == cnt[:, 0].astype(np.int64).sum(), (what, r)
        assert np.array_equal(cnt[:, 0], cnt[:, 3:].sum(1)) and cnt[:, 1:3].sum() == 0, (what, r)
        assert st[4] == (cnt[:, 0] == 0).sum() and st[5] == cnt[:, 0].max(), (what, r)
        for n in [0] + list(range(3, n_max + 1)):
            assert np.array_equal(mh[n], np.bincount(np.minimum(cnt[:, n], 32), minlength=33)), (what, r, n)
        assert mh[1:3].sum() == 0 and mh[n_max + 1:].sum() == 0, (what, r)
        rows = sorted_rows(ring)
        if st[6] == 0:
            assert len(rows) == st[1] and len(set(rows)) == len(rows), (what, r)
            assert np.array_equal(np.bincount([len(p) for p in rows], minlength=9), rh[0]), (what, r)
        assert all(p[0] == min(p) and p[1] < p[-1] and len(set(p)) == len(p) for p in rows), (what, r)
    # summed outputs, and identical bits from call to call
    assert np.array_equal(tot["ring_hist"], per["ring_hist"].sum(0)), what
    assert np.array_equal(tot["member_hist"], per["member_hist"].sum(0)), what
    assert np.array_equal(tot["stats"], per["stats"]), what
    again = b.hbond_rings(r_hb, theta, n_max, per_replica=True, details=True, max_rings=max_rings)
    for key in KEYS:
        assert np.array_equal(per[key].view(np.uint8), again[key].view(np.uint8)), (what, key)
    assert all(sorted_rows(per["ring"][r]) == sorted_rows(again["ring"][r]) for r in rs), what
    return per, tot, wants


def frames_batch(frames, box):
    a = net.water_arrays(frames[0], box)
    b = make_batch(a, len(frames), rcut=min(RCUT, 0.49 * box))
    for r, c in enumerate(frames):
        ar = net.water_arrays(c, box)
        b.set_replica(r, ar["com"], ar["coords"])
    b.recip_long()
    return b


def variants(c, box, seed):
    """The frame, the frame moved as a whole and folded back into the box (bonds now cross its faces:
    other box vectors, the same rings), and the frame with its molecules relabelled."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(c) // 3)
    return [c, net.translated(c, rng.random(3) * box, box), net.permuted(c, perm)], perm


@pytest.mark.parametrize("n_mol,wgs", [(2, 0), (3, 0), (5, 0), (64, 0), (65, 0), (65, 1), (129, 0)])
def test_small_and_odd_systems(n_mol, wgs):
    """The minimum of two, no ring possible (2), one lane pass (64), a second pass with one molecule
    (65), three passes (129); mixed atom types, so the SoA arrays are read.  Wide criteria make rings
    in a thin random system: (6 A, 50 degrees) gives 65 molecules 74 rings and 45 wrapping ones, and
    flags 129 molecules (13 bonds) beside (5 A, 40 degrees), which does not."""
    box = 22.0
    a = small_system(n_mol, box, seed=300 + n_mol)
    with make_batch(a, 3) as b:
        shifted_replicas(b, a, box)
        b.set_option("wave_wgs", wgs)                          # 1: one workgroup takes the three replicas in turn
        per5, _, w5 = check_batch(b, [box] * 3, 5.0, 40.0, what=f"n_mol {n_mol}, 5 A")
        per6, _, w6 = check_batch(b, [box] * 3, 6.0, 50.0, what=f"n_mol {n_mol}, 6 A")
        assert np.all(per5["stats"][:, 7] == 0)
        if n_mol == 65:
            assert per6["stats"][0, 1] > 50 and per6["stats"][0, 2] > 20
        if n_mol == 129:
            assert np.all(per6["stats"][:, 7] == 1) and per5["stats"][0, 1] > 20


def test_candidate_lists_longer_than_a_wave():
    """129 molecules in a 22 A box and r_hb = L / 2: most molecules have more than 64 oxygens inside
    the gate (up to 90), so a candidate list is worked off inside the scan and its rest moved down.
    A cone of 10 degrees leaves at most 6 partners: nothing is flagged, and lists, donations and
    rings are compared with the restatement's."""
    import local_order_ref
    box = 22.0
    a = small_system(129, box, seed=429)
    with make_batch(a, 3) as b:
        shifted_replicas(b, a, box)
        for r in range(3):
            _, r2 = local_order_ref.oo_vectors(b.get_replica(r)[1], box)
            assert ((r2 < 121.0).sum(1) - 1).max() > 64
        per, _, _ = check_batch(b, [box] * 3, 11.0, 10.0, what="r_hb L/2")
        assert np.all(per["stats"][:, 7] == 0) and np.all(per["stats"][:, 0] > 100) and np.all(per["stats"][:, 1] > 0)


def test_one_molecule_is_refused():
    a = small_system(1, 22.0, seed=7)
    with make_batch(a, 2) as b:
        out = sentinels(b, 4)
        with pytest.raises(_lib.MMCError) as ei:
            b.hbond_rings(details=True, max_rings=4, out=out)
        assert ei.value.status == _lib.MMC_ERR_UNSUPPORTED and untouched(out)


def test_the_largest_system_and_one_molecule_more():
    """MMC_NET_MAX_MOL = 2048 molecules: partner indices use all eleven bits of a list entry and the
    level arrays of sixteen waves fill the LDS; at (5.5 A, 50 degrees) a molecule has exactly the
    eight bonds a list holds.  2049 are refused."""
    box = 56.0
    a = small_system(net.MAX_MOL, box, seed=2048)
    with make_batch(a, 2) as b:
        shifted_replicas(b, a, box)
        per, _, wants = check_batch(b, [box] * 2, 5.5, 50.0, replicas=[1], what="2048")
        assert wants[1]["A"].sum(1).max() == ref.MAX_DEG and wants[1]["stats"][1] > 1000
        assert np.array_equal(per["stats"][0], per["stats"][1])  # replica 1 is replica 0 moved as a whole
    a = small_system(net.MAX_MOL + 1, box, seed=2049)
    with make_batch(a, 2) as b:
        out = sentinels(b, 4)
        with pytest.raises(_lib.MMCError) as ei:
            b.hbond_rings(details=True, max_rings=4, out=out)
        assert ei.value.status == _lib.MMC_ERR_UNSUPPORTED and untouched(out)


@pytest.mark.parametrize("nc", [2, 3])
def test_ice_ic(nc):
    """Proton-ordered cubic ice: 2 N six-rings, every molecule in twelve, nothing else -- but in the
    box of 2^3 cells also 912 eight-rings that close through the box, in the row of their own."""
    c, box = ref.ice_ic(nc)
    n = len(c) // 3
    frames, _ = variants(c, box, seed=nc)
    with frames_batch(frames, box) as b:
        per, _, _ = check_batch(b, [box] * 3, what=f"ice {nc}")
        for r in range(3):
            want = np.zeros((3, 9), dtype=np.uint64)
            want[0, 6] = 2 * n
            want[1, 8] = 912 if nc == 2 else 0
            assert np.array_equal(per["ring_hist"][r], want), (r, per["ring_hist"][r])
            assert np.all(per["count"][r, :, 0] == 12) and np.all(per["count"][r, :, 6] == 12)
            assert list(per["stats"][r]) == [2 * n, 2 * n, want[1, 8], 0, 0, 12, 0, 0]


def test_seven_rings_wrapping_homodromic_and_not():
    """Four frames of seven waters in a box of 20 A: the closed line through the box (one wrapping
    7-ring, nothing in row 0), the planar heptagon whose waters each donate to the next (homodromic),
    the same with one bond donated both ways (still homodromic), and that one after the double donor
    is turned away from its second partner (a 7-ring that is not homodromic)."""
    box = 20.0
    frames = [net.torus_line(7, 0, box), ref.polygon(7, box), ref.polygon(7, box, "ff2ffff"), ref.polygon(7, box, "ffbffff")]
    with frames_batch(frames, box) as b:
        per, _, _ = check_batch(b, [box] * 4, 3.1, 30.0, what="heptagons")
        assert [list(per["ring_hist"][r, :, 7]) for r in range(4)] == [[0, 1, 0], [1, 0, 1], [1, 0, 1], [1, 0, 0]]
        assert np.all(per["ring_hist"][:, :2].sum((1, 2)) == 1)
        assert np.all(per["count"][0] == 0) and np.all(per["count"][1:, :, 7] == 1)


@pytest.mark.parametrize("name", ["squares", "cube", "octagon"])
def test_polycyclic_frames(name):
    """Two squares sharing an edge (the 6-cycle round both has a shortcut of one bond), the cube (its
    six-cycles over three faces fall to a common partner, its eight-cycles to the test at ring
    distance 4, four six-rings stay) and the octagon with a bridge of three bonds (two 7-rings; the
    octagon itself falls to the bridge): each depth of the shortcut test.  Each frame also moved
    across the faces of the box and relabelled."""
    box = 20.0
    c = getattr(ref, name + "_frame")(box)
    frames, perm = variants(c, box, seed=len(c))
    with frames_batch(frames, box) as b:
        per, _, wants = check_batch(b, [box] * 3, 3.1, 30.0, what=name)
        want = {"squares": {4: 2}, "cube": {4: 6, 6: 4}, "octagon": {7: 2}}[name]
        for r in range(3):
            assert {n: int(v) for n, v in enumerate(per["ring_hist"][r, 0]) if v} == want and per["stats"][r, 2] == 0
        inv = np.argsort(perm)
        mapped = sorted(canonical(tuple(int(inv[m]) for m in p)) for p in wants[0]["rows"])
        assert mapped == sorted_rows(per["ring"][2])


def canonical(p):
    k = p.index(min(p))
    q = p[k:] + p[:k]
    return q if q[1] < q[-1] else (q[0],) + q[:0:-1]


@pytest.mark.parametrize("variant", ["unwrapped", "reference"])
def test_nist_config_1_in_both_com_conventions(variant):
    a = common.nist_arrays(1, variant)
    with make_batch(a, 3) as b:
        b.run(150, T, 0.4, 0.2, seed=2, n_groups=1)            # replicas diverge
        per, _, _ = check_batch(b, [a["box"]] * 3, what=variant)
        assert per["stats"][:, 1].min() > 20 and not np.array_equal(per["count"][0], per["count"][1])


def test_750_molecules_at_two_criteria():
    a = common.nist_arrays(4, "unwrapped")
    with make_batch(a, 3) as b:
        b.set_option("device_moves", 1)
        b.run(300, T, DR, DPHI, seed=4242)
        per, _, _ = check_batch(b, [a["box"]] * 3, what="cfg4")
        dense, _, _ = check_batch(b, [a["box"]] * 3, 3.6, 40.0, replicas=[2], what="cfg4, dense")
        assert per["stats"][:, 1].min() > 50 and np.all(dense["stats"][:, 0] > per["stats"][:, 0])
        from metropolismontecarlo_amd import observables as obs
        assert np.isclose(obs.ring_fractions(per["ring_hist"].sum(0)).sum(), 1.0)


def test_a_flagged_replica_beside_exact_ones():
    """Ten waters: nine donors round a central acceptor flag the replica; the replicas beside it (the
    bridged octagon, also ten) are exact."""
    box = 20.0
    flagged = nine_donors(box)
    want = ref.rings(flagged, box, 3.1, cosd(30.0))
    assert want["A"].sum(1).max() == 9 and want["stats"][7] == 1
    octagon = ref.octagon_frame(box)
    with frames_batch([octagon, flagged, net.translated(octagon, [9.0, 3.0, 11.0], box)], box) as b:
        per, tot, _ = check_batch(b, [box] * 3, 3.1, 30.0, what="flag")
        assert list(per["stats"][:, 7]) == [0, 1, 0] and np.all(per["count"][1] == 65535) and np.all(per["ring"][1] == -1)
        assert np.array_equal(per["ring_hist"][0], per["ring_hist"][2]) and per["ring_hist"][0, 0, 7] == 2
        assert tot["ring_hist"][0, 7] == 4


def nine_donors(box):
    """A water in the middle of the box and nine at 2.8 A round it (three rings of three, staggered)
    whose first hydrogens point at it."""
    mid = np.full(3, box / 2)
    O = [mid]
    for ring, (polar, turn) in enumerate(((45.0, 0.0), (90.0, 60.0), (135.0, 0.0))):
        for k in range(3):
            th, ph = np.deg2rad(polar), np.deg2rad(turn + 120.0 * k)
            O.append(mid + 2.8 * np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)]))
    return ref.donor_frame(O, [(k, 0) for k in range(1, 10)], box, r_hb=3.1, check=False)


def test_overflow_of_the_ring_list():
    a = common.nist_arrays(1, "unwrapped")
    with make_batch(a, 2) as b:
        b.run(150, T, 0.4, 0.2, seed=2, n_groups=1)
        wants = [ref.rings(b.get_replica(r)[1], a["box"]) for r in range(2)]
        few = min(len(w["rows"]) for w in wants) - 5
        assert few > 10
        out = b.hbond_rings(per_replica=True, details=True, max_rings=few)
        for r, want in enumerate(wants):
            assert out["stats"][r, 6] == len(want["rows"]) - few
            rows = sorted_rows(out["ring"][r])
            assert len(rows) == few and len(set(rows)) == few and set(rows) <= set(want["rows"])
            stats = want["stats"].copy()
            stats[6] = len(want["rows"]) - few
            assert np.array_equal(out["stats"][r], stats)
            for key in ("ring_hist", "member_hist", "count"):
                assert np.array_equal(out[key][r], want[key]), (r, key)


def test_n_max_truncates_and_changes_no_smaller_ring():
    a = common.nist_arrays(1, "unwrapped")
    with make_batch(a, 2) as b:
        b.run(150, T, 0.4, 0.2, seed=2, n_groups=1)
        full, _, _ = check_batch(b, [a["box"]] * 2, n_max=8, what="n_max 8")
        for n_max in (3, 6):
            per, _, _ = check_batch(b, [a["box"]] * 2, n_max=n_max, what=f"n_max {n_max}")
            assert np.array_equal(per["ring_hist"][:, :, :n_max + 1], full["ring_hist"][:, :, :n_max + 1])
            assert np.array_equal(per["count"][:, :, 3:n_max + 1], full["count"][:, :, 3:n_max + 1])
            assert np.array_equal(per["member_hist"][:, 3:n_max + 1], full["member_hist"][:, 3:n_max + 1])
        assert full["ring_hist"][:, 0, 7:].sum() > 0


def test_per_replica_boxes():
    states = per_box_states([0.97, 1.0, 1.04])
    with per_box_batch(states) as b:
        e0 = b.potential_ewald(as_array=True)["energy"].copy()
        b.run_npt_replicas(2, T, 0.0024, 300.0, DR, DPHI, seed=9, energies=e0, moves_per_sweep=40)
        boxes = b.get_boxes()
        assert len(set(boxes)) == 3
        per, _, _ = check_batch(b, boxes, what="per box")
        assert per["stats"][:, 1].min() > 20
        out = sentinels(b, 4)
        with pytest.raises(_lib.MMCError) as ei:
            b.hbond_rings(np.nextafter(0.5 * boxes.min(), 100.0), details=True, max_rings=4, out=out)
        assert ei.value.status == _lib.MMC_ERR_ARG and untouched(out)


def test_wolf_style():
    a = common.nist_arrays(1, "unwrapped")
    with make_batch(a, 3) as b:
        b.set_option("device_moves", 1)
        b.set_coulomb_style("wolf")
        e = b.potential_wolf(as_array=True)["energy"].copy()
        b.run(90, T, 0.4, 0.2, seed=8, energies=e)
        per, _, _ = check_batch(b, [a["box"]] * 3, what="wolf")
        assert not np.array_equal(per["count"][0], per["count"][1])


def test_the_array_path_equals_the_record_path():
    """The same coordinates in a batch whose Ewald parameters keep it off the 128-byte records
    (kappa above the table's range): the kernel reads the SoA arrays and must count the same rings."""
    from metropolismontecarlo_amd.device import Batch
    a = common.nist_arrays(1, "unwrapped")
    with make_batch(a, 3) as b:
        b.run(150, T, 0.4, 0.2, seed=2, n_groups=1)
        rec = b.hbond_rings(per_replica=True, details=True)
        states = [b.get_replica(r) for r in range(3)]
    with Batch(3, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"], 12.0 / a["box"],
               structs.factor, RCUT, RCUT) as b:
        for r, (com, coords, *_) in enumerate(states):
            b.set_replica(r, com, coords)
        b.recip_long()
        arr, _, _ = check_batch(b, [a["box"]] * 3, what="arrays")
    for key in KEYS:
        assert np.array_equal(arr[key], rec[key]), key
    assert rec["stats"][:, 1].min() > 20


@pytest.mark.parametrize("system", ["records", "arrays"])
def test_launch_shape_does_not_change_the_results(system):
    n_cus = common.device_cu_count()
    R = 10 * n_cus + 1                                      # every workgroup of the default grid takes several replicas
    a = common.nist_arrays(1, "unwrapped") if system == "records" else small_system(65, 22.0, seed=17)
    crit = (3.5, 30.0) if system == "records" else (6.0, 50.0)
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
        some = sorted({0, 1, R // 2, R - 1})
        base_per, base_tot, wants = check_batch(b, [a["box"]] * R, *crit, replicas=some, what=system)
        assert base_per["stats"][:, 6].sum() == 0 and base_per["stats"][:, 1].min() > 10
        if system == "records":
            assert not np.array_equal(base_per["count"][0], base_per["count"][R - 1])
        max_rings = base_per["ring"].shape[1]
        for wgs, chunk in ((16, 0), (50, R // 3 + 1), (0, 0)):       # (one workgroup alone: test_small_and_odd_systems)
            b.set_option("wave_wgs", wgs)
            b.set_option("ring_chunk", chunk)                  # three launches, the last one ragged
            per = b.hbond_rings(*crit, per_replica=True, details=True, max_rings=max_rings)
            tot = b.hbond_rings(*crit)
            for k in KEYS:
                assert np.array_equal(per[k].view(np.uint8), base_per[k].view(np.uint8)), (system, wgs, k)
            for k in base_tot:
                assert np.array_equal(tot[k].view(np.uint8), base_tot[k].view(np.uint8)), (system, wgs, k)
            for r in some + [2, R - 2]:
                assert sorted_rows(per["ring"][r]) == sorted_rows(base_per["ring"][r]), (system, wgs, r)


def chain(b, interleave, n_blocks=2, steps=60):
    e = b.potential_ewald(as_array=True)["energy"].copy()
    stats = []
    for blk in range(n_blocks):
        e, st = b.run(steps, T, DR, DPHI, seed=21, energies=e)
        stats.append({k: v for k, v in st.items() if isinstance(v, int)})
        if interleave:
            b.hbond_rings(3.5, 30.0, 8 - 2 * blk, per_replica=bool(blk & 1), details=bool(blk & 1), max_rings=300 * (blk & 1))
    return e, stats, [b.get_replica(r) for r in range(b.R)]


def test_calls_between_blocks_leave_the_chain_bit_identical():
    """Coordinates, S(k) (get_replica's third array) and energies of 2 x 60 steps with a call after
    each block, against the same chain without."""
    a = common.nist_arrays(4, "unwrapped")
    runs = []
    for interleave in (False, True):
        with make_batch(a, 6) as b:
            b.set_option("device_moves", 1)
            runs.append(chain(b, interleave))
    x, y = runs
    assert np.array_equal(x[0].view(np.uint64), y[0].view(np.uint64))
    assert x[1] == y[1]
    for p, q in zip(x[2], y[2]):
        assert all(np.array_equal(u.view(np.uint8), v.view(np.uint8)) for u, v in zip(p, q))


def sentinels(b, max_rings, per_replica=False):
    R, N = b.R, b.n_mol
    lead = (R,) if per_replica else ()
    return dict(ring_hist=np.full(lead + (3, 9), 99, dtype=np.uint64), member_hist=np.full(lead + (9, 33), 99, dtype=np.uint64),
                stats=np.full((R, 8), -7, dtype=np.int64), count=np.full((R, N, 9), 5, dtype=np.uint16),
                ring=np.full((R, max_rings, 8), -5, dtype=np.int32))


def untouched(out):
    return (np.all(out["ring_hist"] == 99) and np.all(out["member_hist"] == 99) and np.all(out["stats"] == -7)
            and np.all(out["count"] == 5) and np.all(out["ring"] == -5))


def test_refusals_leave_outputs_untouched():
    a = common.nist_arrays(1, "unwrapped")
    R = 2
    L = _lib.lib()

    def expect(status, b, per=False, **kw):
        out = sentinels(b, 4, per)
        with pytest.raises(_lib.MMCError) as ei:
            b.hbond_rings(per_replica=per, details=True, max_rings=4, out=out, **kw)
        assert ei.value.status == status and untouched(out), kw

    with make_batch(a, R) as b:
        # proposals outstanding
        com, coords = np.asarray(a["com"]), np.asarray(a["coords"])
        b.eval(np.full(R, 3), np.tile(com[2], (R, 1)), np.tile(coords[6:9], (R, 1, 1)))
        expect(_lib.MMC_ERR_STATE, b)
        expect(_lib.MMC_ERR_STATE, b, per=True)
        b.settle(np.zeros(R, dtype=np.int32))
        # bad arguments
        for r_hb in (float("nan"), float("inf"), -float("inf"), 0.0, -3.5, np.nextafter(a["box"] / 2, 100.0)):
            expect(_lib.MMC_ERR_ARG, b, r_hb=r_hb)
        for theta in (120.0, 180.0, float("nan")):             # cos_hb <= 0 or NaN
            expect(_lib.MMC_ERR_ARG, b, theta_deg=theta)
        for n_max in (2, 9, -1):
            expect(_lib.MMC_ERR_ARG, b, n_max=n_max, per=True)
        st = np.full((R, 8), -7, dtype=np.int64)
        ring = np.full((R, 4, 8), -5, dtype=np.int32)
        p64, p32 = st.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int64)), ring.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32))
        for cos_hb in (0.0, -0.2, np.nextafter(1.0, 2.0), float("nan")):
            assert L.mmc_batch_hbond_rings(b._h, 3.5, cos_hb, 8, 0, None, None, p64, None, 0, None) == _lib.MMC_ERR_ARG
        assert L.mmc_batch_hbond_rings(b._h, 3.5, 0.8, 8, 0, None, None, None, None, 0, None) == _lib.MMC_ERR_ARG
        for max_rings in (0, -1):
            assert L.mmc_batch_hbond_rings(b._h, 3.5, 0.8, 8, 0, None, None, p64, None, max_rings, p32) == _lib.MMC_ERR_ARG
        assert np.all(st == -7) and np.all(ring == -5)
        # ... and after all that the call works, r_hb = L / 2 and cos_hb = 1 exactly included, with one output
        # only; max_rings is ignored without ring_out
        assert L.mmc_batch_hbond_rings(b._h, a["box"] / 2, 1.0, 3, 0, None, None, p64, None, -1, None) == _lib.MMC_OK
        assert np.all(st[:, 7] == 0) and np.all(st[:, 6] == 0)
        assert np.array_equal(b.hbond_rings(a["box"] / 2, 0.0, 3)["stats"], st)
    # a volume trial in flight
    with per_box_batch(per_box_states([1.0, 1.02])) as b:
        boxes = b.get_boxes()
        b.volume_trial_replicas(boxes * np.array([1.01, 0.0]))
        expect(_lib.MMC_ERR_STATE, b)
        b.volume_settle(np.zeros(R, dtype=np.int32))
        assert b.hbond_rings()["stats"][:, 0].min() > 0
