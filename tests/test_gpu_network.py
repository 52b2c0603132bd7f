"""mmc_batch_hbond_network against its numpy restatement (tests/network_ref.py).

Every output is an integer and must be equal exactly: the bonds (nbr), the degrees, the labels, the
cluster sizes, the wrap masks and the seven sums, per replica and summed, from call to call and
whatever the launch shape.

Launch shape: a replica is a workgroup's unit; workgroup g of G takes the replicas g, g + G, ...
G is option "wave_wgs", by default what is resident.  The criteria of a call are worked off in
groups as the LDS holds them, so several criteria in one call also cross the boundary between two
passes over the molecules where the system is large (750 molecules: at most five per pass)."""
import numpy as np
import pytest

import common
import network_ref as ref
from metropolismontecarlo_amd import _lib, structs

pytestmark = pytest.mark.gpu

RCUT = 10.0
T, DR, DPHI = 298.15, 0.3, 0.2
ALPHA = 5.6
KEYS = ("size_hist", "deg_hist", "stats", "label", "nbr")


def make_batch(a, R, rcut=RCUT):
    from metropolismontecarlo_amd.device import Batch
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
              ALPHA / a["box"], structs.factor, rcut, rcut)
    b.recip_long()
    return b


def split(crit):
    r_hb, theta, minb = (list(x) for x in zip(*crit))
    return dict(r_hb=r_hb, theta_deg=theta, min_bonds=minb)


def check_batch(b, boxes, crit=((3.5, 30.0, 0),), replicas=None, what=""):
    """One detailed per-replica call and one summed call against the restatement of every replica in
    `replicas` (default all), against each other and against the identities between the outputs."""
    R, N, K = b.R, b.n_mol, len(crit)
    per = b.hbond_network(per_replica=True, details=True, **split(crit))
    tot = b.hbond_network(**split(crit))
    assert per["size_hist"].shape == (R, K, N + 1) and per["deg_hist"].shape == (R, K, 17)
    assert tot["size_hist"].shape == (K, N + 1) and tot["deg_hist"].shape == (K, 17)
    assert per["stats"].shape == (R, K, 8) and per["label"].shape == (R, K, N) and per["nbr"].shape == (R, K, N, 16)
    wants = {}
    for r in (range(R) if replicas is None else replicas):
        coords = b.get_replica(r)[1]
        for k, (r_hb, theta, minb) in enumerate(crit):
            want = ref.network(coords, float(boxes[r]), r_hb, float(np.cos(np.deg2rad(float(theta)))), minb)
            wants[r, k] = want
            for key in KEYS:
                assert np.array_equal(per[key][r, k], want[key]), (what, r, k, key, per["stats"][r, k], want["stats"])
    for r in range(R):                                          # the identities between the device's own outputs
        for k in range(K):
            st, sh, lab, nbr = per["stats"][r, k], per["size_hist"][r, k], per["label"][r, k], per["nbr"][r, k]
            s = np.arange(N + 1, dtype=np.uint64)
            assert (sh * s).sum() == st[1] and sh.sum() == st[2] and sh[0] == 0, (what, r, k)
            if st[7]:
                assert list(st[:7]) == [0] * 7 and np.all(lab == -2) and np.all(nbr == -1), (what, r, k)
                assert sh.sum() == 0 and per["deg_hist"][r, k].sum() == 0, (what, r, k)
                continue
            roots, counts = np.unique(lab[lab >= 0], return_counts=True)
            assert np.array_equal(np.bincount(counts, minlength=N + 1), sh), (what, r, k)
            assert np.all(lab[roots] == roots) and (st[4] == (counts.astype(np.int64) ** 2).sum()), (what, r, k)
            deg = (nbr >= 0).sum(1)
            assert np.array_equal(np.bincount(deg, minlength=17), per["deg_hist"][r, k]), (what, r, k)
            assert deg.sum() == 2 * st[0] and np.array_equal(lab >= 0, deg >= crit[k][2]), (what, r, k)
            assert st[3] == (counts.max() if len(counts) else 0) and st[6] <= st[3] and (st[6] > 0) == (st[5] != 0)
    # summed outputs, and identical bits from call to call
    assert np.array_equal(tot["size_hist"], per["size_hist"].sum(0)), what
    assert np.array_equal(tot["deg_hist"], per["deg_hist"].sum(0)), what
    assert np.array_equal(tot["stats"], per["stats"]), what
    again = b.hbond_network(per_replica=True, details=True, **split(crit))
    for key in per:
        assert np.array_equal(per[key].view(np.uint8), again[key].view(np.uint8)), (what, key)
    return per, tot, wants


def small_system(n_mol, box, seed):
    return common.random_system(n_mol, box, seed=seed, na_choices=(3,))


def shifted_replicas(b, a, box):
    for r in range(1, b.R):                                    # replicas differ
        sh = np.random.default_rng(r).random(3) * box
        b.set_replica(r, (a["com"] + sh) % box, a["coords"] + np.repeat((a["com"] + sh) % box - a["com"], 3, axis=0))
    b.recip_long()


@pytest.mark.parametrize("n_mol", [2, 3, 64, 65, 129])
def test_small_and_odd_systems(n_mol):
    """The minimum of two, one lane pass (64), a second pass with one molecule (65), three passes
    (129); mixed atom types, so the SoA arrays are read.  r_hb = 7 makes dozens of candidates per
    molecule, and min_bonds = 2 cuts sites out of the same bonds; at 129 molecules a molecule has 18
    partners there, so those two criteria are flagged beside one that is not."""
    box = 22.0
    a = small_system(n_mol, box, seed=300 + n_mol)
    with make_batch(a, 3) as b:
        shifted_replicas(b, a, box)
        per, _, wants = check_batch(b, [box] * 3, ((3.5, 30.0, 0), (7.0, 50.0, 0), (7.0, 50.0, 2)), what=f"n_mol {n_mol}")
        assert np.array_equal(per["nbr"][:, 1], per["nbr"][:, 2])
        if n_mol >= 64:
            assert wants[0, 1]["A"].sum() > 0 and np.all(per["stats"][:, 0, 7] == 0)


def test_candidate_lists_longer_than_a_wave():
    """129 molecules in a 22 A box and r_hb = L / 2: most molecules have more than 64 oxygens inside
    the gate (up to 90), so a candidate list is worked off inside the scan and its rest moved down.
    A cone of 12 degrees leaves at most 9 partners: nothing is flagged, and the lists are compared
    entry by entry -- beside a criterion of 3.5 A in the same pass over the molecules."""
    import local_order_ref
    box = 22.0
    a = small_system(129, box, seed=429)
    with make_batch(a, 3) as b:
        shifted_replicas(b, a, box)
        for r in range(3):
            _, r2 = local_order_ref.oo_vectors(b.get_replica(r)[1], box)
            assert ((r2 < 121.0).sum(1) - 1).max() > 64
        per, _, wants = check_batch(b, [box] * 3, ((11.0, 12.0, 0), (3.5, 30.0, 0)), what="r_hb L/2")
        assert np.all(per["stats"][:, :, 7] == 0) and wants[0, 0]["A"].sum(1).max() > 4


def test_one_molecule_is_refused():
    a = small_system(1, 22.0, seed=7)
    with make_batch(a, 2) as b:
        out = sentinels(b, 1)
        with pytest.raises(_lib.MMCError) as ei:
            b.hbond_network(details=True, out=out)
        assert ei.value.status == _lib.MMC_ERR_UNSUPPORTED
        assert untouched(out)


def test_the_largest_system_and_one_molecule_more():
    """MMC_NET_MAX_MOL = 2048 molecules: partner indices use all eleven bits of a list entry, the
    lists of one criterion fill the LDS (one criterion per pass over the molecules, sixteen waves),
    and a cluster of nearly all molecules puts the sum of s^2 at 2^22.  2049 are refused."""
    box = 56.0
    a = small_system(ref.MAX_MOL, box, seed=2048)
    with make_batch(a, 2) as b:
        shifted_replicas(b, a, box)
        per, _, wants = check_batch(b, [box] * 2, ((6.0, 50.0, 3), (4.0, 40.0, 0)), replicas=[1], what="2048")
        assert wants[1, 0]["stats"][3] > 1024 and wants[1, 0]["stats"][5] == 7 and per["nbr"][1].max() == ref.MAX_MOL - 1
        assert np.array_equal(per["stats"][0], per["stats"][1])  # replica 1 is replica 0 moved as a whole
    a = small_system(ref.MAX_MOL + 1, box, seed=2049)
    with make_batch(a, 2) as b:
        out = sentinels(b, 1)
        with pytest.raises(_lib.MMCError) as ei:
            b.hbond_network(details=True, out=out)
        assert ei.value.status == _lib.MMC_ERR_UNSUPPORTED and untouched(out)


def line_frames(n, p, box, seed):
    """The intact and the broken torus line, each also under a random permutation of the molecules
    and under a random rigid translation folded back into the box."""
    rng = np.random.default_rng(seed)
    frames = []
    for broken in (False, True):
        c = ref.torus_line(n, p, box, broken)
        perm = rng.permutation(n)
        frames += [(broken, None, c), (broken, perm, ref.permuted(c, perm)),
                   (broken, None, ref.translated(c, rng.random(3) * box, box))]
    return frames


@pytest.mark.parametrize("n,p,box", [(129, 8, 44.8), (65, 4, 45.3)])
def test_propagation_longer_than_a_wave_is_wide(n, p, box):
    """A path of n - 1 bonds whose lowest index sits at one end: the label 0 needs n - 1 rounds, more
    than a wave has lanes (129) or exactly as many (65); intact, the line winds p times along x and
    once along y, never along z.  Six frames as six replicas of one batch."""
    frames = line_frames(n, p, box, seed=n)
    a = ref.water_arrays(frames[0][2], box)
    with make_batch(a, len(frames)) as b:
        for r, (_, _, c) in enumerate(frames):
            ar = ref.water_arrays(c, box)
            b.set_replica(r, ar["com"], ar["coords"])
        b.recip_long()
        per, _, wants = check_batch(b, [box] * len(frames), ((3.5, 30.0, 0), (3.5, 30.0, 2)), what=f"line {n}")
        for r, (broken, perm, _) in enumerate(frames):
            bonds, mask = (n - 1, 0) if broken else (n, 3)
            assert list(per["stats"][r, 0]) == [bonds, n, 1, n, n * n, mask, n if mask else 0, 0], (r, per["stats"][r, 0])
            assert np.all(per["label"][r, 0] == 0)
            want = wants[r, 0]
            rounds = ref.propagation_rounds(want["A"], np.ones(n, dtype=bool), want["label"])
            if broken and perm is None:
                assert rounds >= n - 1                           # the graph's diameter, from the far end
            if perm is not None:                               # the partners follow the permutation
                inv = np.argsort(perm)
                base = per["nbr"][r - 1, 0]
                for k in range(n):
                    assert set(per["nbr"][r, 0, k][per["nbr"][r, 0, k] >= 0]) == set(inv[base[perm[k]][base[perm[k]] >= 0]])
        # min_bonds = 2 on the broken line: its two ends are no sites, the rest is one path
        assert list(per["stats"][3, 1, :4]) == [n - 1, n - 2, 1, n - 2] and per["stats"][3, 1, 5] == 0


@pytest.mark.parametrize("variant", ["unwrapped", "reference"])
def test_nist_config_1_in_both_com_conventions(variant):
    a = common.nist_arrays(1, variant)
    with make_batch(a, 3) as b:
        b.run(150, T, 0.4, 0.2, seed=2, n_groups=1)            # replicas diverge
        per, tot, _ = check_batch(b, [a["box"]] * 3, ((3.5, 30.0, 0), (3.2, 30.0, 0), (3.5, 30.0, 3)), what=variant)
        assert not np.array_equal(per["nbr"][0], per["nbr"][1])
        assert per["stats"][:, 0, 0].min() > 50                 # water: bonds are there


EXAMPLE_R_HB = (2.9, 3.0, 3.1, 3.2, 3.3, 3.4, 3.5, 3.6)


def test_750_molecules_nine_criteria_in_two_calls():
    """The example's eight criteria in one call (two passes over the molecules), and the
    four-bonded patches."""
    a = common.nist_arrays(4, "unwrapped")
    with make_batch(a, 3) as b:
        b.set_option("device_moves", 1)
        b.run(300, T, DR, DPHI, seed=4242)
        crit = tuple((r, 30.0, 0) for r in EXAMPLE_R_HB)
        per, tot, wants = check_batch(b, [a["box"]] * 3, crit, what="cfg4")
        assert any(wants[r, 6]["stats"][5] == 7 for r in range(3))    # 3.5 A: some replica wraps x, y and z
        assert np.any(per["stats"][:, 6, 5] == 7)
        per2, _, wants2 = check_batch(b, [a["box"]] * 3, ((3.5, 30.0, 4), (2.9, 20.0, 0)), what="cfg4, patches")
        assert all(wants2[r, 1]["stats"][5] == 0 for r in range(3))   # 2.9 A, 20 deg: nothing wraps
        assert np.all(per2["stats"][:, 1, 5] == 0) and np.all(per2["stats"][:, 1, 6] == 0)
        assert np.array_equal(per2["nbr"][:, 0], per["nbr"][:, 6])    # the same bonds, fewer sites
        assert 0 < per2["stats"][0, 0, 1] < 750
        from metropolismontecarlo_amd import observables as obs
        p_any, p_all = obs.percolation_probability(per["stats"])
        assert p_any[6] > 0 and p_all[6] > 0
        assert np.all(np.isfinite(obs.mean_cluster_size(tot["size_hist"], tot["stats"])))


def test_flagged_criteria_leave_the_others_alone():
    a = common.nist_arrays(1, "unwrapped")
    with make_batch(a, 3) as b:
        b.run(150, T, 0.4, 0.2, seed=2, n_groups=1)
        per, tot, wants = check_batch(b, [a["box"]] * 3, ((4.5, 60.0, 0), (7.0, 75.0, 0), (3.5, 30.0, 0), (7.0, 75.0, 4)),
                                      what="flagged")
        for r in range(3):
            assert wants[r, 0]["stats"][7] == 0 and wants[r, 0]["A"].sum(1).max() <= 16
            assert wants[r, 1]["A"].sum(1).max() > 16
        assert np.all(per["stats"][:, [1, 3], 7] == 1) and np.all(per["stats"][:, [0, 2], 7] == 0)
        assert np.all(per["label"][:, [1, 3]] == -2) and np.all(per["nbr"][:, [1, 3]] == -1)
        assert tot["size_hist"][[1, 3]].sum() == 0 and tot["deg_hist"][[1, 3]].sum() == 0
        alone = b.hbond_network(3.5, 30.0, 0, per_replica=True, details=True)
        for key in KEYS:
            assert np.array_equal(alone[key][:, 0], per[key][:, 2]), key


def test_unbonded_molecules_are_local_orders():
    a = common.nist_arrays(1, "unwrapped")
    with make_batch(a, 3) as b:
        b.run(150, T, 0.4, 0.2, seed=5, n_groups=1)
        unbonded = 0
        for r_hb, theta in ((3.5, 30.0), (3.0, 20.0), (2.8, 15.0)):
            net = b.hbond_network(r_hb, theta, per_replica=True, details=True)
            hb = b.local_order(10, r_hb, theta, details=True)["hb"].astype(int)
            deg = (net["nbr"][:, 0] >= 0).sum(-1)
            assert np.array_equal(deg == 0, hb.sum(-1) == 0)
            assert np.any(deg > 0)
            unbonded += int((deg == 0).sum())
        assert unbonded > 0


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
        e0 = b.potential_ewald(as_array=True)["energy"].copy()
        b.run_npt_replicas(2, T, 0.0024, 300.0, DR, DPHI, seed=9, energies=e0, moves_per_sweep=40)
        boxes = b.get_boxes()
        assert len(set(boxes)) == 3
        half = 0.5 * boxes.min()
        per, _, _ = check_batch(b, boxes, ((3.5, 30.0, 0), (half, 4.0, 0), (3.3, 30.0, 3)), what="per box")
        assert per["stats"][:, 1, 7].sum() == 0 and per["stats"][:, 1, 0].min() > 0   # half the smallest box, a narrow cone
        out = sentinels(b, 1)
        with pytest.raises(_lib.MMCError) as ei:
            b.hbond_network(np.nextafter(half, 100.0), details=True, out=out)
        assert ei.value.status == _lib.MMC_ERR_ARG and untouched(out)


def test_wolf_style():
    a = common.nist_arrays(1, "unwrapped")
    with make_batch(a, 3) as b:
        b.set_option("device_moves", 1)
        b.set_coulomb_style("wolf")
        e = b.potential_wolf(as_array=True)["energy"].copy()
        b.run(90, T, 0.4, 0.2, seed=8, energies=e)
        per, _, _ = check_batch(b, [a["box"]] * 3, ((3.5, 30.0, 0), (3.5, 30.0, 4)), what="wolf")
        assert not np.array_equal(per["label"][0], per["label"][1])


@pytest.mark.parametrize("system", ["records", "arrays"])
def test_launch_shape_does_not_change_the_results(system):
    n_cus = common.device_cu_count()
    R = 10 * n_cus + 1                                      # every workgroup of the default grid takes several replicas
    a = common.nist_arrays(1, "unwrapped") if system == "records" else small_system(65, 22.0, seed=17)
    crit = ((3.5, 30.0, 0), (3.2, 30.0, 2)) if system == "records" else ((7.0, 50.0, 0), (7.0, 50.0, 2))
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
        base_per, base_tot, _ = check_batch(b, [a["box"]] * R, crit, replicas=some, what=system)
        if system == "records":
            assert not np.array_equal(base_per["nbr"][0], base_per["nbr"][R - 1])
        for wgs in (1, 3, 0):
            b.set_option("wave_wgs", wgs)
            per = b.hbond_network(per_replica=True, details=True, **split(crit))
            tot = b.hbond_network(**split(crit))
            for k in base_per:
                assert np.array_equal(per[k].view(np.uint8), base_per[k].view(np.uint8)), (system, wgs, k)
            for k in base_tot:
                assert np.array_equal(tot[k].view(np.uint8), base_tot[k].view(np.uint8)), (system, wgs, k)


def chain(b, interleave, n_blocks=2, steps=60):
    e = b.potential_ewald(as_array=True)["energy"].copy()
    stats = []
    for blk in range(n_blocks):
        e, st = b.run(steps, T, DR, DPHI, seed=21, energies=e)
        stats.append({k: v for k, v in st.items() if isinstance(v, int)})
        if interleave:
            b.hbond_network((3.5, 3.0), 30.0, (0, 4), per_replica=bool(blk & 1), details=bool(blk & 1))
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


def sentinels(b, K, per_replica=False):
    R, N = b.R, b.n_mol
    lead = (R,) if per_replica else ()
    return dict(size_hist=np.full(lead + (K, N + 1), 99, dtype=np.uint64), deg_hist=np.full(lead + (K, 17), 99, dtype=np.uint64),
                stats=np.full((R, K, 8), -7, dtype=np.int64), label=np.full((R, K, N), -5, dtype=np.int32),
                nbr=np.full((R, K, N, 16), -5, dtype=np.int32))


def untouched(out):
    return (np.all(out["size_hist"] == 99) and np.all(out["deg_hist"] == 99) and np.all(out["stats"] == -7)
            and np.all(out["label"] == -5) and np.all(out["nbr"] == -5))


def test_refusals_leave_outputs_untouched():
    a = common.nist_arrays(1, "unwrapped")
    R = 2
    L = _lib.lib()

    def expect(status, b, per=False, **kw):
        K = len(np.atleast_1d(kw.get("r_hb", 3.5)))
        out = sentinels(b, K, per)
        with pytest.raises(_lib.MMCError) as ei:
            b.hbond_network(per_replica=per, details=True, out=out, **kw)
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
            expect(_lib.MMC_ERR_ARG, b, r_hb=(3.5, r_hb), per=True)
        for theta in (120.0, 180.0, float("nan")):             # cos_hb <= 0 or NaN
            expect(_lib.MMC_ERR_ARG, b, theta_deg=theta)
        for minb in (-1, 17):
            expect(_lib.MMC_ERR_ARG, b, min_bonds=minb)
        expect(_lib.MMC_ERR_ARG, b, r_hb=[3.5] * 9)
        st = np.full((R, 1, 8), -7, dtype=np.int64)
        p64 = st.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int64))
        one_d, one_i = (_lib.C.c_double * 1), (_lib.C.c_int32 * 1)
        for cos_hb in (0.0, -0.2, np.nextafter(1.0, 2.0), float("nan")):
            assert L.mmc_batch_hbond_network(b._h, 1, one_d(3.5), one_d(cos_hb), one_i(0), 0, None, None, p64,
                                             None, None) == _lib.MMC_ERR_ARG
        assert L.mmc_batch_hbond_network(b._h, 1, one_d(3.5), one_d(0.8), one_i(0), 0, None, None, None,
                                         None, None) == _lib.MMC_ERR_ARG
        assert L.mmc_batch_hbond_network(b._h, 1, None, one_d(0.8), one_i(0), 0, None, None, p64, None, None) == _lib.MMC_ERR_ARG
        assert np.all(st == -7)
        # ... and after all that the call works, r_hb = L / 2 and cos_hb = 1 exactly included, with one output only
        assert L.mmc_batch_hbond_network(b._h, 1, one_d(a["box"] / 2), one_d(1.0), one_i(0), 0, None, None, p64,
                                         None, None) == _lib.MMC_OK
        assert np.all(st[:, 0, 7] == 0) and np.all(st[:, 0, 1] == b.n_mol)
        assert np.array_equal(b.hbond_network(a["box"] / 2, 0.0)["stats"], st)
    # a volume trial in flight
    with per_box_batch(per_box_states([1.0, 1.02])) as b:
        boxes = b.get_boxes()
        b.volume_trial_replicas(boxes * np.array([1.01, 0.0]))
        expect(_lib.MMC_ERR_STATE, b)
        b.volume_settle(np.zeros(R, dtype=np.int32))
        assert b.hbond_network()["stats"][:, 0, 1].sum() == R * b.n_mol
