"""mmc_batch_bond_order against its numpy restatement (tests/bond_order_ref.py).

Everything is compared exactly: the five histograms, stats, nbr, ab and label as integers; q, qbar and
sums bit for bit (NaN where the restatement has NaN) -- every operation between the coordinates and
these values is a correctly rounded + - x / or sqrt in the header's order, with nothing fused, and the
sums are k_local_qsum's fixed tree, restated here.  What the frames cover, and the known answers of
the lattices, are asserted on the restatement by test_bond_order_host.py.

Launch shape: the unit of phases A and B is a molecule; workgroup g of G takes the molecules
[n N g / G, n N (g + 1) / G) of a chunk of n replicas and its waves share the run's molecules of one
replica after the other.  G is option "wave_wgs", n option "bond_chunk"."""
import numpy as np
import pytest

import bond_order_ref as ref
import common
import shell_order_ref as sref
from metropolismontecarlo_amd import _lib, structs

pytestmark = pytest.mark.gpu

RCUT = 10.0
T, DR, DPHI = 298.15, 0.3, 0.2
ALPHA = 5.6
INF = float("inf")


def make_batch(a, R, rcut=RCUT):
    from metropolismontecarlo_amd.device import Batch
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
              ALPHA / a["box"], structs.factor, rcut, rcut)
    b.recip_long()
    return b


def same_bits(dev, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(dev), nan) and np.array_equal(dev[~nan].view(np.uint64), want[~nan].view(np.uint64))


def qsum(q):
    """k_local_qsum: lane l adds the finite q of molecules l, l + 64, ... in that order; the 64 lane
    sums by an inclusive scan inside each row of 16 (steps 1, 2, 4, 8; zero from beyond the row) and
    the four row totals in row order."""
    acc, cnt = np.zeros(64), 0
    for i, v in enumerate(q):
        if np.isfinite(v):
            acc[i % 64] = acc[i % 64] + v
            cnt += 1
    v = acc.reshape(4, 16)
    for s in (1, 2, 4, 8):
        sh = np.zeros_like(v)
        sh[:, s:] = v[:, :-s]
        v = v + sh
    r = v[:, 15]
    return ((r[0] + r[1]) + r[2]) + r[3], float(cnt)


def check_batch(b, boxes, p=None, replicas=None, what=""):
    """One detailed per-replica call and one summed call against the restatement of every replica
    in `replicas` (default all) and against each other; returns (per, tot, [restatements])."""
    p = ref.params() if p is None else p
    R, N = b.R, b.n_mol
    per = b.bond_order(**p, per_replica=True, details=True)
    tot = b.bond_order(**p)
    shapes = dict(q_hist=(p["q_bins"] + 1,), qbar_hist=(p["q_bins"] + 1,), c_hist=(p["c_bins"] + 1,), ab_hist=(17, 17),
                  size_hist=(N + 1,))
    for k, s in shapes.items():
        assert per[k].shape == (R,) + s and tot[k].shape == s and per[k].dtype == np.uint64
    assert per["stats"].shape == (R, 8) and per["stats"].dtype == np.int64 and per["sums"].shape == (R, 4)
    assert per["q"].shape == (R, N) and per["qbar"].shape == (R, N) and per["nbr"].shape == (R, N, 16)
    assert per["ab"].shape == (R, N, 2) and per["ab"].dtype == np.uint8 and per["label"].shape == (R, N)
    wants = []
    for r in (range(R) if replicas is None else replicas):
        want = ref.bond_order(b.get_replica(r)[1], float(boxes[r]), **p)
        wants.append(want)
        for k in ("nbr", "ab", "label", "stats") + ref.HISTS:
            assert np.array_equal(per[k][r], want[k]), (what, r, k)
        for k in ("q", "qbar"):
            assert same_bits(per[k][r], want[k]), (what, r, k, np.nanmax(np.abs(per[k][r] - want[k])))
    for r in range(R):                                         # every replica: the outputs against each other
        st = per["stats"][r]
        assert st[0] + st[1] + st[2] == N and per["q_hist"][r].sum() == N and per["qbar_hist"][r].sum() == N, (what, r)
        assert per["ab_hist"][r].sum() == st[0] and per["q_hist"][r, :-1].sum() == st[0], (what, r)
        assert per["c_hist"][r].sum() == np.count_nonzero(per["nbr"][r] >= 0), (what, r)
        assert st[4] == np.count_nonzero(per["label"][r] >= 0) == (per["size_hist"][r] * np.arange(N + 1, dtype=np.uint64)).sum()
        assert st[5] == per["size_hist"][r].sum() and st[7] == (per["size_hist"][r] * np.arange(N + 1, dtype=np.uint64) ** 2).sum()
        sq, nq = qsum(per["q"][r])
        sb, nb = qsum(per["qbar"][r])
        assert same_bits(per["sums"][r], np.array([sq, nq, sb, nb])), (what, r)
    # summed outputs, and identical bits from call to call
    for k in ref.HISTS:
        assert np.array_equal(tot[k], per[k].sum(0)), (what, k)
    assert np.array_equal(tot["stats"], per["stats"]), what
    assert np.array_equal(tot["sums"].view(np.uint64), per["sums"].view(np.uint64)), what
    again = b.bond_order(**p, per_replica=True, details=True)
    for k in per:
        assert np.array_equal(per[k].view(np.uint8), again[k].view(np.uint8)), (what, k)
    return per, tot, wants


R_NB = {4: 3.7, 12: 7.0, 16: 0.5 * sref.BOX}


@pytest.mark.parametrize("n_mol", ref.SIZES)
def test_small_and_odd_systems(n_mol):
    """Two, three, one lane pass (64), a second pass with one and two molecules (65, 66), three passes
    (129); mixed atom types, so the SoA arrays are read; three replicas that differ.  l = 3, 4, 6 with
    4, 12 and 16 neighbours inside 3.7 A, 7 A and L / 2, and bin counts 200, 7 and 4096: at 129
    molecules and L / 2 some molecules are flagged and others have bonds to them."""
    a = sref.random_frame(n_mol)
    with make_batch(a, 3) as b:
        for r in (1, 2):
            b.set_replica(r, *sref.replica_frame(a, r))
        b.recip_long()
        bins = {4: 200, 12: 7, 16: 4096}
        to_flagged = False
        for stage in (1, 0):                                   # staged in LDS; read from device memory
            b.set_option("local_stage", stage)
            for l in (3, 4, 6):
                for n_nb in (4, 12, 16):
                    if stage == 0 and (l, n_nb) not in ((3, 4), (4, 12), (6, 16)):
                        continue
                    p = ref.params(l=l, n_nb=n_nb, r_nb=R_NB[n_nb], min_a=1, min_ab=2, a=(-1.0, -0.3), b=(0.2, INF),
                                   q_bins=bins[n_nb], c_bins=bins[n_nb])
                    _, _, wants = check_batch(b, [sref.BOX] * 3, p, what=f"n_mol {n_mol}, l {l}, n_nb {n_nb}, stage {stage}")
                    for w in wants:
                        f = w["flagged"]
                        to_flagged |= bool(np.any(w["used"] & f[np.maximum(w["nbr"], 0)] & ~f[:, None]))
        assert to_flagged == (n_mol == 129)


def test_lattices():
    """Simple cubic (q4, q6), fcc (q6, q4), diamond (every c3 staggered, one cluster of 64) and the
    wurtzite fragment (three staggered bonds and an eclipsed one at the centre) through the kernels;
    the values are test_bond_order_host.py's, from the Legendre form."""
    a, r_nb = ref.sc_frame()
    with make_batch(a, 2) as b:
        per, _, _ = check_batch(b, [a["box"]] * 2, ref.params(l=4, n_nb=6, r_nb=r_nb), what="sc, l 4")
        assert np.abs(per["q"] - 0.763763).max() < 1e-6
        per, _, _ = check_batch(b, [a["box"]] * 2, ref.params(l=6, n_nb=6, r_nb=r_nb), what="sc, l 6")
        assert np.abs(per["q"] - 0.353553).max() < 1e-6
    a, r_nb = ref.fcc_frame()
    with make_batch(a, 2) as b:
        per, _, _ = check_batch(b, [a["box"]] * 2, ref.params(l=6, n_nb=12, r_nb=r_nb), what="fcc, l 6")
        assert np.abs(per["q"] - 0.574524).max() < 1e-6 and np.abs(per["qbar"] - 0.574524).max() < 1e-6
        per, _, _ = check_batch(b, [a["box"]] * 2, ref.params(l=4, n_nb=12, r_nb=r_nb), what="fcc, l 4")
        assert np.abs(per["q"] - 0.190941).max() < 1e-6
    a, r_nb = ref.diamond_frame()
    with make_batch(a, 2) as b:
        per, tot, _ = check_batch(b, [a["box"]] * 2, ref.params(r_nb=r_nb), what="diamond")
        assert tot["ab_hist"][4, 0] == 128 and tot["size_hist"][64] == 2 and tot["c_hist"][:20].sum() == 2 * 64 * 4
        assert per["stats"].tolist() == [[64, 0, 0, 0, 64, 1, 64, 4096]] * 2 and np.all(per["label"] == 0)
    a = ref.wurtzite_fragment()
    with make_batch(a, 2) as b:
        per, _, _ = check_batch(b, [a["box"]] * 2, what="wurtzite")
        assert per["ab"][0, 0].tolist() == [3, 1] and per["nbr"][0, 0, :4].tolist() == [1, 2, 3, 4]


@pytest.mark.parametrize("n_mol", [65, 66])
def test_oxygens_in_a_ball_fill_the_list_exactly_or_flag_everything(n_mol):
    a = sref.ball_frame(n_mol)
    with make_batch(a, 2) as b:
        for stage in (1, 0):
            b.set_option("local_stage", stage)
            per, tot, _ = check_batch(b, [sref.BOX] * 2, ref.params(r_nb=6.0, n_nb=16, l=6), what=f"ball {n_mol}, stage {stage}")
            if n_mol == 65:
                assert np.all(per["stats"][:, [0, 2, 3]] == [65, 0, 65]) and np.all(per["nbr"] >= 0)
            else:
                assert np.all(per["stats"] == [0, 0, 66, 0, 0, 0, 0, 0]) and np.all(per["nbr"] == -1)
                assert tot["q_hist"][-1] == 2 * 66 and tot["c_hist"].sum() == 0 and np.all(np.isnan(per["q"]))
                assert np.all(per["sums"] == 0.0) and np.all(per["label"] == -1)


def test_coincident_oxygens_are_undefined_and_in_no_bin():
    a = sref.coincident_frame()
    with make_batch(a, 2) as b:
        for l, n_nb in ((3, 4), (6, 16)):
            per, _, (want, _) = check_batch(b, [sref.BOX] * 2, ref.params(l=l, n_nb=n_nb, r_nb=6.0), what="coincident")
            assert per["nbr"][0, 0, 0] == 1 and per["nbr"][0, 1, 0] == 0 and np.all(np.isnan(per["q"][0, :2]))
            lonely = np.count_nonzero(per["nbr"][0, :, 0] < 0)
            assert per["stats"][0, 1] == 2 + lonely and per["q_hist"][0, -1] == 2 + lonely
            assert per["c_hist"][0, -1] >= np.count_nonzero(per["nbr"][0, :2] >= 0) and per["c_hist"][0, :-1].sum() > 0
            assert np.all(per["label"][0, :2] == -1)


def test_more_neighbours_in_range_than_asked_for_are_counted_as_truncated():
    a = common.nist_arrays(1, "unwrapped")
    with make_batch(a, 2) as b:
        per, _, _ = check_batch(b, [a["box"]] * 2, ref.params(n_nb=4, r_nb=6.0), what="truncated")
        assert per["stats"][0, 3] > 50 and np.all(per["nbr"][:, :, 4:] == -1)


def test_a_line_of_128_is_one_cluster():
    """Index 0 at one end, two neighbours each: the label 0 has 127 bonds to travel."""
    a = ref.line_frame()
    with make_batch(a, 2) as b:
        per, _, _ = check_batch(b, [a["box"]] * 2, ref.params(n_nb=2, min_a=0, min_ab=0), what="line")
        assert per["stats"].tolist() == [[128, 0, 0, 0, 128, 1, 128, 128 * 128]] * 2 and np.all(per["label"] == 0)


def test_edges_listed_from_one_end_only_join_their_molecules():
    a = ref.bridging_frame()
    with make_batch(a, 2) as b:
        per, _, _ = check_batch(b, [a["box"]] * 2, ref.params(n_nb=1, min_a=0, min_ab=0), what="bridging")
        assert per["label"][0].tolist() == [0] * 6 + [6] * 6 and per["stats"][0, 4:].tolist() == [12, 2, 6, 72]


def test_one_molecule_is_refused():
    a = sref.random_frame(1)
    with make_batch(a, 2) as b:
        out = sentinels(b, ref.params())
        with pytest.raises(_lib.MMCError) as ei:
            b.bond_order(details=True, out=out)
        assert ei.value.status == _lib.MMC_ERR_UNSUPPORTED and untouched(out)
        assert "N = 1" in str(ei.value)


TEN_WOLDE = ref.params(l=6, n_nb=16, r_nb=3.5, a=(0.5, 1.0), min_a=7, min_ab=0)


@pytest.mark.parametrize("variant", ["unwrapped", "reference"])
def test_nist_config_1_in_both_com_conventions(variant):
    a = common.nist_arrays(1, variant)
    with make_batch(a, 3) as b:
        b.run(150, T, 0.4, 0.2, seed=2, n_groups=1)            # replicas diverge
        per, tot, _ = check_batch(b, [a["box"]] * 3, what=variant)
        assert not np.array_equal(per["nbr"][0], per["nbr"][1]) and np.isfinite(per["q"]).sum() > 250
        b.set_option("local_stage", 0)
        check_batch(b, [a["box"]] * 3, TEN_WOLDE, what=variant + ", q6 criterion, unstaged")


def test_750_molecules():
    a = common.nist_arrays(4, "unwrapped")
    with make_batch(a, 3) as b:
        b.set_option("device_moves", 1)
        b.run(300, T, DR, DPHI, seed=4242)
        per, tot, _ = check_batch(b, [a["box"]] * 3, what="cfg4")
        from metropolismontecarlo_amd import observables as obs
        assert per["stats"][:, 2].sum() == 0 and np.all(obs.solid_fraction(per["stats"]) < 0.2)   # a liquid
        assert obs.chill_plus_classes(per).sum(1).tolist() == [750] * 3
        check_batch(b, [a["box"]] * 3, ref.params(l=6, n_nb=12, r_nb=4.5, a=(0.5, 1.0), min_a=2, min_ab=0), replicas=[1],
                    what="cfg4, l 6")


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
        per, _, _ = check_batch(b, boxes, what="per box")
        assert not np.array_equal(per["q_hist"][0], per["q_hist"][2])
        half = 0.5 * boxes.min()
        out = sentinels(b, ref.params())
        with pytest.raises(_lib.MMCError) as ei:
            b.bond_order(r_nb=np.nextafter(half, 100.0), details=True, out=out)
        assert ei.value.status == _lib.MMC_ERR_ARG and untouched(out)


def test_wolf_style():
    a = common.nist_arrays(1, "unwrapped")
    with make_batch(a, 3) as b:
        b.set_option("device_moves", 1)
        b.set_coulomb_style("wolf")
        e = b.potential_wolf(as_array=True)["energy"].copy()
        b.run(90, T, 0.4, 0.2, seed=8, energies=e)
        per, _, _ = check_batch(b, [a["box"]] * 3, what="wolf")
        assert not np.array_equal(per["q"][0].view(np.uint64), per["q"][1].view(np.uint64))


@pytest.mark.parametrize("system", ["records", "arrays"])
def test_launch_shape_and_chunking_do_not_change_the_results(system):
    """wave_wgs 1, 2 and the default, positions staged or not, and chunks of 2 replicas of 5 (a
    ragged last chunk), of 1 and of more than there are."""
    R = 5
    a = common.nist_arrays(1, "unwrapped") if system == "records" else sref.random_frame(65, seed=17)
    p = ref.params(r_nb=4.5, n_nb=6, min_a=1, min_ab=2, a=(-1.0, -0.4), b=(-0.4, 0.4))
    with make_batch(a, R) as b:
        if system == "records":
            b.set_option("device_moves", 1)
            b.run(30, T, 0.4, 0.2, seed=11)
        else:
            for r in range(1, R):
                b.set_replica(r, *sref.replica_frame(a, r))
            b.recip_long()
        base_per, base_tot, _ = check_batch(b, [a["box"]] * R, p, what=system)
        assert not np.array_equal(base_per["nbr"][0], base_per["nbr"][R - 1]) and base_per["stats"][:, 4].sum() > 0
        for wgs, stage, chunk in ((1, 1, 0), (2, 1, 0), (0, 0, 0), (1, 0, 2), (0, 1, 2), (2, 1, 1), (0, 1, 7)):
            b.set_option("wave_wgs", wgs)
            b.set_option("local_stage", stage)
            b.set_option("bond_chunk", chunk)
            per = b.bond_order(**p, per_replica=True, details=True)
            tot = b.bond_order(**p)
            for k in base_per:
                assert np.array_equal(per[k].view(np.uint8), base_per[k].view(np.uint8)), (system, wgs, stage, chunk, k)
            for k in base_tot:
                assert np.array_equal(tot[k].view(np.uint8), base_tot[k].view(np.uint8)), (system, wgs, stage, chunk, k)
        with pytest.raises(_lib.MMCError):
            b.set_option("bond_chunk", -1)


def test_null_outputs_cost_nothing_and_change_nothing():
    """Each output alone through the C call -- so the neighbour phase alone, the first two phases,
    and all three -- gives the numbers of the full call."""
    a = common.nist_arrays(1, "unwrapped")
    C = _lib.C
    kinds = dict(q_hist=C.c_uint64, qbar_hist=C.c_uint64, c_hist=C.c_uint64, ab_hist=C.c_uint64, size_hist=C.c_uint64,
                 stats=C.c_int64, sums=C.c_double, q=C.c_double, qbar=C.c_double, nbr=C.c_int32, ab=C.c_uint8,
                 label=C.c_int32)
    with make_batch(a, 2) as b:
        p = ref.params(min_a=1, min_ab=2)
        full = b.bond_order(**p, details=True)
        for pos, (k, ct) in enumerate(kinds.items()):
            got = np.full_like(full[k], 3)
            ptrs = [None] * 12
            ptrs[pos] = got.ctypes.data_as(C.POINTER(ct))
            st = _lib.lib().mmc_batch_bond_order(b._h, p["l"], p["r_nb"], p["n_nb"], p["a"][0], p["a"][1], p["b"][0],
                                                 p["b"][1], p["min_a"], p["min_ab"], p["q_bins"], p["c_bins"], 0, *ptrs)
            assert st == _lib.MMC_OK and np.array_equal(got.view(np.uint8), full[k].view(np.uint8)), k


def chain(b, interleave, n_blocks=2, steps=60):
    e = b.potential_ewald(as_array=True)["energy"].copy()
    stats = []
    for blk in range(n_blocks):
        e, st = b.run(steps, T, DR, DPHI, seed=21, energies=e)
        stats.append({k: v for k, v in st.items() if isinstance(v, int)})
        if interleave:
            b.bond_order(per_replica=bool(blk & 1), details=bool(blk & 1))
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


def sentinels(b, p, per_replica=False):
    R, N = b.R, b.n_mol
    lead = (R,) if per_replica else ()
    nq, nc = (max(int(p[k]), 0) for k in ("q_bins", "c_bins"))
    return dict(q_hist=np.full(lead + (nq + 1,), 99, dtype=np.uint64), qbar_hist=np.full(lead + (nq + 1,), 99, dtype=np.uint64),
                c_hist=np.full(lead + (nc + 1,), 99, dtype=np.uint64), ab_hist=np.full(lead + (17, 17), 99, dtype=np.uint64),
                size_hist=np.full(lead + (N + 1,), 99, dtype=np.uint64), stats=np.full((R, 8), 99, dtype=np.int64),
                sums=np.full((R, 4), 7.5), q=np.full((R, N), 7.5), qbar=np.full((R, N), 7.5),
                nbr=np.full((R, N, 16), -5, dtype=np.int32), ab=np.full((R, N, 2), 9, dtype=np.uint8),
                label=np.full((R, N), -5, dtype=np.int32))


def untouched(out):
    return (all(np.all(out[k] == 99) for k in ref.HISTS + ("stats",)) and all(np.all(out[k] == 7.5) for k in ("sums", "q", "qbar"))
            and np.all(out["nbr"] == -5) and np.all(out["ab"] == 9) and np.all(out["label"] == -5))


def test_refusals_leave_outputs_untouched():
    a = common.nist_arrays(1, "unwrapped")
    R = 2

    def expect(status, bt, per=False, **kw):
        p = ref.params(**kw)
        out = sentinels(bt, p, per)
        with pytest.raises(_lib.MMCError) as ei:
            bt.bond_order(**p, per_replica=per, details=True, out=out)
        assert ei.value.status == status and untouched(out), kw

    with make_batch(a, R) as b:
        # proposals outstanding
        com, coords = np.asarray(a["com"]), np.asarray(a["coords"])
        b.eval(np.full(R, 3), np.tile(com[2], (R, 1)), np.tile(coords[6:9], (R, 1, 1)))
        expect(_lib.MMC_ERR_STATE, b)
        expect(_lib.MMC_ERR_STATE, b, per=True)
        b.settle(np.zeros(R, dtype=np.int32))
        # bad arguments
        nan = float("nan")
        for kw in (dict(l=5), dict(l=0), dict(n_nb=0), dict(n_nb=17), dict(r_nb=nan), dict(r_nb=INF), dict(r_nb=0.0),
                   dict(r_nb=-3.5), dict(r_nb=np.nextafter(a["box"] / 2, 100.0)), dict(q_bins=-1), dict(c_bins=-1),
                   dict(q_bins=4097), dict(a=(nan, 0.0)), dict(a=(-1.0, nan)), dict(b=(nan, 0.0)), dict(b=(0.0, nan))):
            expect(_lib.MMC_ERR_ARG, b, **kw)
            expect(_lib.MMC_ERR_ARG, b, per=True, **kw)
        # ... and after all that the call works: the limits themselves, r_nb = L / 2, infinite windows
        res = b.bond_order(l=6, n_nb=16, r_nb=a["box"] / 2, a=(-INF, INF), b=(-INF, INF), q_bins=4096, c_bins=4096)
        assert res["q_hist"].sum() == R * b.n_mol
    # a volume trial in flight
    with per_box_batch(per_box_states([1.0, 1.02])) as b:
        boxes = b.get_boxes()
        b.volume_trial_replicas(boxes * np.array([1.01, 0.0]))
        expect(_lib.MMC_ERR_STATE, b)
        b.volume_settle(np.zeros(R, dtype=np.int32))
        res = b.bond_order()
        assert res["q_hist"].sum() == R * b.n_mol
