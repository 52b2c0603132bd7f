"""Forces and torques (mmc_batch_forces) on the rest of what k_forces_wave reads or branches on, against
the numpy restatement forces_ref.molecule (tests/test_gpu_forces.py has the definition, the sums, the
flags and the refusals; tests/test_forces_paths_host.py pins the restatement on the oracle at these
inputs and asserts their geometry on a machine without a GPU):
  1. the neighbour list emptied mid-scan, so that f[9], a_v, a_w and the overlap mask add across the
     process() calls of one unit -- k_forces_wave's pair body and scan are its own code;
  2. separate LJ and Coulomb cutoffs (same_gate == false), with the per-molecule and the per-pair
     image, the latter with atom pairs between the two slacks;
  3. the cold series below r^2 = 0.25 in a wave whose other lanes are on the table, the table's first
     node to the bit, and the overlap radius to the bit (r^2 = 0.5 is no overlap, the double under it is);
  4. the committed state -- coordinates, records, S buffer, box, kappa -- after every path that
     changes it; there S(k) is also recomputed on the host (forces_ref.oracle_S: the oracle's
     RecipLong on get_replica's coordinates), so that a stale S buffer shows even where get_replica
     would return the same stale one;
  5. small and odd sizes: the scan's tail masks, the prefetch past n_mol, idle lanes, N = 1 refused;
  6. the per-molecule image against the per-pair image on one configuration.
Tolerance per value: forces_ref.close, 1e-12 A + 1e-300; overlap flags exact; fsum and n_flagged bit
for bit forces_ref.host_sums of the returned rows.

Record of one run on an MI355X, the worst |x - ref| / A per item (the bound is 1e-12): 1. 7.8e-16;
2. 9.3e-16; 3. 1.1e-15 at the contact and 2.2e-15 at the thresholds; 4. 1.0e-15, with the host's S(k)
as with get_replica's; 5. 2.2e-15; 6. 1.1e-15, and every row of the two images byte-identical.  The 26
cases took 4.3 s together, the slowest (N = 385, all molecules of three replicas) 1.2 s."""
import ctypes as C

import numpy as np
import pytest

import common
import forces_ref as ref
import solute_ref
from test_gpu_deletion import edge_selection
from test_gpu_deletion_paths import make_batch

pytestmark = pytest.mark.gpu

T = 298.15
RC = 10.0
MASS = np.array([15.9994, 1.00794, 1.00794])
SEL8 = np.array([0, 63, 64, 301, 302, 511, 700, 749])
SEL16 = np.array([0, 1, 63, 64, 65, 127, 128, 200, 255, 256, 301, 400, 512, 640, 700, 749])
ROWS = ("force", "torque", "vir", "atom", "ovl", "fsum", "n_flagged")


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def cfg4():
    return common.nist_arrays(4, "unwrapped")


def check_selected(orc, a, b, sel, what, lj=RC, qq=RC, host_s=True, out=None):
    """One call for the molecules sel of every replica, all rows with masses: every value against the
    restatement on get_replica's coordinates -- with get_replica's S(k) and, host_s, with the
    oracle's S(k) of those coordinates -- in the box of get_boxes; fsum and n_flagged against the
    fixed-order host sums of the returned rows.  Returns (the call's dict, worst |x - ref| / A)."""
    sel = np.asarray(sel)
    out = b.forces(sel=sel, mass=MASS, details=True) if out is None else out
    box = float(b.get_boxes()[0])
    su = ref.setup(a, orc, box, lj, qq)
    rows = np.arange(sel.shape[0])
    worst = 0.0
    for r in range(b.R):
        worst = max(worst, ref.check(su, b, r, sel, out, rows, MASS, what=what))
        if host_s:
            S = ref.oracle_S(orc, a, b.get_replica(r)[1], box)
            worst = max(worst, ref.check(su, b, r, sel, out, rows, MASS, what=(what, "host S"), S=S))
    fsum, nfl = ref.host_sums(out["force"], out["torque"], out["vir"], out["ovl"])
    assert out["fsum"].tobytes() == fsum.tobytes(), what
    assert np.array_equal(out["n_flagged"], nfl), what
    print(what, "worst |x - ref| / A:", worst)
    return out, worst


def same_bytes(x, y):
    return all(x[k].tobytes() == y[k].tobytes() for k in ROWS)


def raw_forces(b, n_sel=0, sel=None, mass=MASS):
    """The C entry point with all seven outputs given and filled with sentinels: (status, whether every
    output still holds its sentinel)."""
    from metropolismontecarlo_amd import _lib
    R, nn = b.R, max(b.n_mol if sel is None else len(sel), 1)
    outs = [np.full((R, nn, 3), -1.5), np.full((R, nn, 3), -1.5), np.full((R, nn, 3), -1.5),
            np.full((R, nn, 9), -1.5), np.full((R, 9), 7.5)]
    nf, ovl = np.full(R, 3, dtype=np.int64), np.full((R, nn), 9, dtype=np.uint8)
    sel_a = None if sel is None else np.ascontiguousarray(sel, dtype=np.int32)
    mass_a = np.ascontiguousarray(mass, dtype=np.float64)
    st = _lib.lib().mmc_batch_forces(
        b._h, n_sel, None if sel_a is None else sel_a.ctypes.data_as(C.POINTER(C.c_int32)),
        mass_a.ctypes.data_as(_lib._dp), *[x.ctypes.data_as(_lib._dp) for x in outs],
        nf.ctypes.data_as(_lib._i64p), ovl.ctypes.data_as(C.POINTER(C.c_uint8)))
    untouched = (all(np.all(x == -1.5) for x in outs[:4]) and np.all(outs[4] == 7.5) and np.all(nf == 3)
                 and np.all(ovl == 9))
    return st, bool(untouched)


# ---- 1. the pair-list flush ---------------------------------------------------------------------
def test_neighbour_list_flush(orc):
    """2000 SPC/E molecules at 0.06 / A^3 with a 12.4 A cutoff (test_gpu_deletion_paths.py's system):
    430-520 COMs inside the gate of any molecule, so the scan of k_forces_wave empties its list at a
    384-molecule trip boundary and goes on (asserted: common.scan_flushes, the molecule itself left
    out).  The nine force sums, both virial sums and the overlap mask must add across process() calls.
    Second call: one opposite-charge overlap (r^2 = 0.3) between molecule i, which meets its partner
    AFTER its first flush, and molecule j, which meets its partner BEFORE its first flush and flushes
    afterwards (forces_ref.flush_overlap_ok, from the COM order and the trip boundaries): both carry
    bit 0 and zero rows and are left out of fsum."""
    a, rc, sel = ref.flush_system()
    L, com = float(a["box"]), np.asarray(a["com"])
    assert sel.shape == (24,)
    for i in sel:
        assert common.scan_flushes(com, [com[i]], rc, L, exclude=int(i)), i
    with make_batch(a, 1, rc, rc) as b:
        out, w1 = check_selected(orc, a, b, sel, "flush", rc, rc, host_s=False)
        assert np.all(out["ovl"] == 0) and np.all(out["fsum"][:, 0] == 24)
        c, i, j = ref.flush_overlap(a, rc)
        assert ref.flush_overlap_ok(c, rc, i, j)
        n_pf = common._wave_list_consts()[1]
        assert i < 64 * n_pf <= ref.first_flush_by(c["com"], i, rc, L) <= j
        b.set_replica(0, c["com"], c["coords"])
        b.recip_long()
        sel2 = np.concatenate([[i, j], sel[:10]])
        assert i not in sel and j not in sel
        for m in sel2:
            assert common.scan_flushes(c["com"], [c["com"][m]], rc, L, exclude=int(m)), m
        out, w2 = check_selected(orc, c, b, sel2, "flush, overlap", rc, rc, host_s=False)
    assert list(out["ovl"][0]) == [1, 1] + [0] * 10
    for k in ("force", "torque", "vir", "atom"):
        assert np.all(out[k][0, :2] == 0.0) and np.any(out[k][0, 2:] != 0.0), k
    assert out["fsum"][0, 0] == 10 and out["n_flagged"][0] == 2


# ---- 2. separate cutoffs ------------------------------------------------------------------------
@pytest.mark.parametrize("lj,qq", [(8.0, 10.0), (10.0, 8.0)])
@pytest.mark.parametrize("variant", ["unwrapped", "reference"])
def test_separate_cutoffs(variant, lj, qq, orc):
    """same_gate == false after 60 device-proposed steps: gl against gq, lon against on, LJ counted
    where Coulomb is not and the reverse.  "unwrapped": the per-molecule image (IMG), the 16 molecules
    at the lane and block edges of deletion's case.  "reference": molecules stored broken across the
    box, the per-pair image, edge_selection's 16 -- whose atom pairs between the two slacks
    (r_cut^2 + 100) are counted on the host: recorded 17 pairs at (8, 10), all charged pairs inside the
    Coulomb gate, and 17 at (10, 8), one of them an LJ pair inside the LJ gate (molecule 302's), the
    pair that `lon` tested against the Coulomb slack would lose."""
    a = common.nist_arrays(4, variant)
    n = np.asarray(a["com"]).shape[0]
    sel = SEL16 if variant == "unwrapped" else edge_selection(n, 16, ref.EDGE_SEED)
    with make_batch(a, 1, lj, qq) as b:
        b.set_option("device_moves", 1)
        b.run(60, T, 0.3, 0.2, seed=99)
        com, coords, _ = b.get_replica(0)
        assert not np.array_equal(com, np.asarray(a["com"]))
        counts = [ref.between_gates(com, int(i), lj, qq, a["box"]) for i in sel]
        assert min(counts) >= 20, counts
        su = ref.setup(a, orc, a["box"], lj, qq)
        n_all, n_lj, n_qq = ref.slack_pairs(su, com, coords, sel)
        print(variant, (lj, qq), "between the gates", min(counts), "..", max(counts),
              "pairs between the slacks:", n_all, "LJ", n_lj, "charged", n_qq)
        if variant == "reference":
            assert n_all > 0 and (n_lj >= 1) == (lj > qq) and (n_qq >= 1) == (qq > lj)
        out, _ = check_selected(orc, a, b, sel, (variant, lj, qq), lj, qq)
        assert np.all(out["ovl"] == 0)


# ---- 3. the cold series and the thresholds ------------------------------------------------------
def test_cold_series_in_a_wave_on_the_table(orc, cfg4):
    """volume_perturb_ref.contact_case on config 4: two hydrogens at r^2 = 0.2, below the erfc table's
    first node and no overlap (like charges).  The contact's two molecules and four others: in the
    contact's round one lane takes qq_pair_cold and the other lanes of the wave the table."""
    a, i, j = ref.contact_system(cfg4, 0.2)
    assert abs(ref.pair_r2(a, i, 1, j, 1) - 0.2) < 1e-12
    assert not ref.opposite_within(a, i) and not ref.opposite_within(a, j)
    assert np.count_nonzero(ref.com_r2(a["com"], i, a["box"]) < RC * RC) - 1 >= 100
    with make_batch(a, 1) as b:
        sel = np.array([i, j, 63, 64, 301, 749])
        out, _ = check_selected(orc, a, b, sel, "contact 0.2")
        assert np.all(out["ovl"] == 0)
        # the contact's force is there: 1.2e5 K/A on each of the two hydrogens, opposite
        f = out["atom"][0, :2, 1]
        assert np.linalg.norm(f[0]) > 1e5 and np.linalg.norm(f[1]) > 1e5 and f[0] @ f[1] < 0


@pytest.mark.parametrize("target,below,atom_i", ref.THRESHOLDS,
                         ids=["like-0.25", "like-under-0.25", "opposite-0.5", "opposite-under-0.5"])
def test_thresholds_to_the_bit(target, below, atom_i, orc, cfg4):
    """One atom pair at a threshold exactly, or at the double just under it (forces_ref.threshold_case:
    the pair vector lies on the coordinate grid, so the kernel's difference is that vector and its
    r^2 that double under any order of evaluation).  Like charges at 0.25: the table's first node,
    and under it the series -- both within tolerance.  Opposite charges at 0.5: no overlap (the
    reference's test is <), evaluated like any pair; under it: both molecules flagged, zero rows."""
    c, i, j, p, u = ref.threshold_case(cfg4, target, below, atom_i)
    assert u == (float(np.nextafter(target, 0.0)) if below else target) == ref.pair_r2(c, i, atom_i, j, 1)
    others = ref.opposite_within(c, j, 0.7)
    assert set(others) <= {i} and not (set(ref.opposite_within(c, i, 0.7)) - {j})
    with make_batch(c, 1) as b:
        sel = np.array([i, j, 63, 64, 301, 749])
        out, _ = check_selected(orc, c, b, sel, ("threshold", target, below))
    flagged = atom_i == 0 and below
    assert list(out["ovl"][0]) == [int(flagged)] * 2 + [0] * 4
    assert np.all(out["atom"][0, :2] == 0.0) == flagged
    assert out["fsum"][0, 0] == (4 if flagged else 6)


# ---- 4. after every path that changes the committed state ---------------------------------------
def test_after_host_decided_runs(cfg4, orc):
    """One step per launch, the host decides (persistent = 0, accept_on_device = 0)."""
    with make_batch(cfg4, 8) as b:
        for k, v in (("device_moves", 1), ("kernel", 2), ("persistent", 0), ("accept_on_device", 0)):
            b.set_option(k, v)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        e, st = b.run(37, T, 0.3, 0.2, seed=5, energies=e)
        assert st["device_decisions"] == 0 and st["trans_accept"] + st["rot_accept"] > 0
        check_selected(orc, cfg4, b, SEL8, "host-decided")


def test_after_kernel_decided_runs(cfg4, orc):
    """Eight steps per launch, the kernel decides, 24 replicas in two groups on one workgroup: the
    rows of every replica, and the chains go on bit for bit like a twin's that made no forces call."""
    R, per_launch = 24, 8
    opts = (("device_moves", 1), ("kernel", 2), ("persistent", 0), ("accept_on_device", 1),
            ("steps_per_launch", per_launch), ("wave_wgs", 1))
    with make_batch(cfg4, R) as b, make_batch(cfg4, R) as tw:
        es = []
        for x in (b, tw):
            for k, v in opts:
                x.set_option(k, v)
            e = x.potential_ewald(as_array=True)["energy"].copy()
            e, st = x.run(3 * per_launch + 5, T, 0.3, 0.2, seed=6, energies=e, n_groups=2, n_parts=1)
            assert st["device_decisions"] == R * (3 * per_launch + 5)
            es.append(e)
        out, _ = check_selected(orc, cfg4, b, SEL8, per_launch)
        assert not np.array_equal(out["force"][0], out["force"][R - 1])
        for x, k in ((b, 0), (tw, 1)):
            es[k], _ = x.run(2 * per_launch + 3, T, 0.3, 0.2, seed=7, energies=es[k], n_groups=2, n_parts=1)
        assert es[0].tobytes() == es[1].tobytes()
        for r in range(R):
            for u, v in zip(b.get_replica(r), tw.get_replica(r)):
                assert np.asarray(u).tobytes() == np.asarray(v).tobytes(), r


def test_after_the_latency_server(cfg4, orc):
    """One replica with the default options: the latency server runs the chain; molecules it moved are
    among the selected."""
    with make_batch(cfg4, 1) as b:
        b.set_option("device_moves", 1)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        e, st = b.run(150, T, 0.3, 0.2, seed=8, energies=e, n_groups=1)
        assert st["server_steps"] == 150
        moved = np.nonzero(np.any(b.get_replica(0)[0] != np.asarray(cfg4["com"]), axis=1))[0]
        assert moved.size >= 4
        check_selected(orc, cfg4, b, np.concatenate([moved[:4], SEL8[:4]]), "latency")


def test_after_eval_and_settle(cfg4, orc):
    """Caller proposals with the host's decisions, one of them accepted: the committed S(k) is in the
    other buffer (s_cur = 1) for every replica; the moved molecule is among the selected."""
    a = cfg4
    R = 2
    com, coords = np.asarray(a["com"]), np.asarray(a["coords"])
    with make_batch(a, R) as b:
        s0 = b.get_replica(1)[2].copy()
        d = np.array([0.2, -0.1, 0.15])
        b.eval(np.full(R, 5), np.tile(com[4] + d, (R, 1)), np.tile(coords[12:15] + d, (R, 1, 1)))
        b.eval(np.full(R, 9), np.tile(com[8] - d, (R, 1)), np.tile(coords[24:27] - d, (R, 1, 1)),
               accept_prev=np.ones(R, dtype=bool))
        b.settle(np.zeros(R, dtype=np.int32))
        c1, x1, s1 = b.get_replica(1)
        assert np.array_equal(c1[4], com[4] + d) and np.array_equal(c1[8], com[8])
        assert not np.array_equal(s0, s1)
        check_selected(orc, a, b, np.array([4, 8, 0, 63, 64, 301, 700, 749]), "eval/settle")


def test_volume_trial_accept_and_reject(cfg4, orc):
    """One replica: between mmc_batch_volume_trial and its decision the call is refused with
    MMC_ERR_STATE and writes nothing; after a reject the same call gives the same bytes as before the
    trial; after an accept to 1.01 V the forces are those of the new box (get_boxes, kappa = 5.6 / box:
    qrec, c_exp, nk2 and the erfc table all follow it)."""
    from metropolismontecarlo_amd import _lib
    a = cfg4
    L1 = (1.01 * a["box"] ** 3) ** (1 / 3)
    with make_batch(a, 1) as b:
        b.set_option("device_moves", 1)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        b.run(80, T, 0.3, 0.2, seed=9, energies=e, n_groups=1)
        before, _ = check_selected(orc, a, b, SEL8, "before the trial")
        for accept in (False, True):
            b.volume_trial(L1, 5.6 / L1)
            st, untouched = raw_forces(b, n_sel=8, sel=SEL8)
            assert st == _lib.MMC_ERR_STATE and untouched
            if accept:
                b.volume_accept()
            else:
                b.volume_reject()
                assert same_bytes(before, b.forces(sel=SEL8, mass=MASS, details=True))
        assert b.get_boxes()[0] == L1
        out, _ = check_selected(orc, a, b, SEL8, "volume accept")
        assert out["atom"].tobytes() != before["atom"].tobytes()


def test_after_run_npt(cfg4, orc):
    """mmc_batch_run_npt on one replica with at least one accepted volume move: the forces in the final
    box of get_boxes()."""
    a = cfg4
    with make_batch(a, 1) as b:
        b.set_option("device_moves", 1)
        e0 = float(b.potential_ewald(as_array=True)["energy"][0])
        e1, st, ns = b.run_npt(8, T, 0.03, 0.05 * a["box"] ** 3, 0.3, 0.2, 13, e0, moves_per_sweep=40)
        assert ns["vol_attempt"] == 8 and ns["vol_accept"] >= 1, ns
        assert b.get_boxes()[0] != a["box"]
        check_selected(orc, a, b, SEL8, ("npt", float(b.get_boxes()[0]), ns["vol_accept"]))


def test_after_set_replica_and_recip_long(cfg4, orc):
    """mmc_batch_set_replica on replica 1 of three, then mmc_batch_recip_long."""
    a = cfg4
    L = float(a["box"])
    com, coords = np.asarray(a["com"]), np.asarray(a["coords"])
    with make_batch(a, 3) as b:
        shift = np.array([1.3, -2.1, 0.4])
        c2 = (com + shift) % L
        x2 = coords + np.repeat(c2 - com, 3, axis=0)
        c2[10] += np.array([0.3, 0.2, -0.1])
        x2[30:33] += np.array([0.3, 0.2, -0.1])
        b.set_replica(1, c2, x2)
        b.recip_long()
        assert np.array_equal(b.get_replica(1)[0], c2)
        out, _ = check_selected(orc, a, b, np.array([10, 0, 63, 64, 301, 511, 700, 749]), "set_replica")
        assert out["force"][0].tobytes() == out["force"][2].tobytes() != out["force"][1].tobytes()


# ---- 5. small and odd sizes ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 129, 385])
def test_small_and_odd_sizes(n, cfg4, orc):
    """The first n molecules of config 4 in its own box, R = 3, each replica shifted rigidly by its
    own vector: every molecule, on one workgroup (wave_wgs = 1: n = 2 gives 6 units on 4 waves) and on
    the default grid, byte for byte the same.  The scan reads WV_PF blocks of 64 ahead of the one it
    tests: the m_end mask, the prefetch past n_mol, idle lanes and the unit's own molecule in its list
    all decide here; 385 ends one molecule past a 384 trip."""
    a = solute_ref.first_molecules(cfg4, n)
    with make_batch(a, 3) as b:
        for r in range(3):
            b.set_replica(r, *ref.shifted_replica(a, r))
        b.recip_long()
        b.set_option("wave_wgs", 1)
        one = b.forces(mass=MASS, details=True)
        b.set_option("wave_wgs", 0)
        out, _ = check_selected(orc, a, b, np.arange(n), ("n", n))
        assert same_bytes(one, out)
        assert np.all(out["ovl"] == 0) and np.all(out["fsum"][:, 0] == n)
        assert not np.array_equal(out["atom"][0], out["atom"][1])


def test_one_molecule_is_refused(cfg4):
    from metropolismontecarlo_amd import _lib
    a = solute_ref.first_molecules(cfg4, 1)
    with make_batch(a, 2) as b:
        st, untouched = raw_forces(b)
        assert st == _lib.MMC_ERR_UNSUPPORTED and untouched
        assert b"at least 2 molecules" in _lib.lib().mmc_last_error()


# ---- 6. the per-molecule image against the per-pair image ---------------------------------------
def test_image_by_molecule_against_per_pair(cfg4, orc):
    """Config 4 "unwrapped" after 60 steps, the same call with option "image_by_molecule" at -1
    (k_forces_wave<true>: where it is valid, and here it is) and at 0 (k_forces_wave<false>): both
    within tolerance of the restatement, the flags identical.  Whether the rows are byte-identical is
    printed, not asserted: the restatement supports the tolerance only."""
    with make_batch(cfg4, 2) as b:
        b.set_option("device_moves", 1)
        b.run(60, T, 0.3, 0.2, seed=99)
        sel = np.concatenate([SEL16, edge_selection(750, 24, 5)])
        img, _ = check_selected(orc, cfg4, b, sel, "image by molecule")
        b.set_option("image_by_molecule", 0)
        per, _ = check_selected(orc, cfg4, b, sel, "image per pair")
        b.set_option("image_by_molecule", -1)
        assert img["ovl"].tobytes() == per["ovl"].tobytes()
        print("rows byte-identical between the two images:", {k: img[k].tobytes() == per[k].tobytes() for k in ROWS})
