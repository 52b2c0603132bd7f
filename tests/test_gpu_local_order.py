"""mmc_batch_local_order against its numpy restatement (tests/local_order_ref.py).

Integers (nbr, hb, hb_hist) must be equal exactly.  q is O(1) and about 30 rounded operations, so
1e-12 absolute leaves room for fused multiply-adds; NaN exactly where the restatement has it.
q_hist must equal the header's bin formula applied on the host to the device's own q (one multiply
and a floor: no bin edge is left to a tolerance).  q_sum[r][0] is within 1e-12 N of the sum of the
device's q and bit-identical between calls; q_sum[r][1] is exact.

Launch shape: k_local_order_wave's unit is a molecule; workgroup g of G takes the molecules
[R N g / G, R N (g + 1) / G) of the replica-major order and its (up to four) waves share the run's
molecules of one replica after the other.  G is option "wave_wgs", by default four workgroups per
compute unit; with wave_wgs = 1 four waves walk every replica, and with R > 2.5 x 4 x n_cus the
default grid gives every wave several molecules of two or three replicas."""
import numpy as np
import pytest

import common
import local_order_ref as ref
from metropolismontecarlo_amd import _lib, structs

pytestmark = pytest.mark.gpu

RCUT = 10.0
T, DR, DPHI = 298.15, 0.3, 0.2
ALPHA = 5.6
Q_TOL = 1e-12


def make_batch(a, R, rcut=RCUT):
    from metropolismontecarlo_amd.device import Batch
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
              ALPHA / a["box"], structs.factor, rcut, rcut)
    b.recip_long()
    return b


def same_q(dev, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(dev), nan) and np.all(np.abs(dev[~nan] - want[~nan]) <= Q_TOL)


def check_batch(b, boxes, q_bins=400, r_hb=3.5, theta=30.0, replicas=None, what=""):
    """One detailed per-replica call and one summed call against the restatement of every replica
    in `replicas` (default all) and against each other."""
    R, N = b.R, b.n_mol
    per = b.local_order(q_bins, r_hb, theta, per_replica=True, details=True)
    tot = b.local_order(q_bins, r_hb, theta)
    assert per["hb_hist"].shape == (R, 3, 9) and per["q_hist"].shape == (R, q_bins)
    assert tot["hb_hist"].shape == (3, 9) and tot["q_hist"].shape == (q_bins,)
    assert per["nbr"].shape == (R, N, 4) and per["q"].shape == (R, N) and per["hb"].shape == (R, N, 2)
    cos_hb = float(np.cos(np.deg2rad(float(theta))))
    for r in (range(R) if replicas is None else replicas):
        want = ref.local_order(b.get_replica(r)[1], float(boxes[r]), r_hb, cos_hb, q_bins)
        assert np.array_equal(per["nbr"][r], want["nbr"]), (what, r)
        assert np.array_equal(per["hb"][r], want["hb"]), (what, r)
        assert np.array_equal(per["hb_hist"][r], want["hb_hist"]), (what, r)
        assert same_q(per["q"][r], want["q"]), (what, r, np.nanmax(np.abs(per["q"][r] - want["q"])))
    for r in range(R):                                         # the device's own q through the host's formulas
        q = per["q"][r]
        assert np.array_equal(per["q_hist"][r], ref.q_histogram(q, q_bins)), (what, r)
        assert np.array_equal(per["hb_hist"][r], ref.hb_histogram(per["hb"][r])), (what, r)
        fin = np.isfinite(q)
        assert per["q_sum"][r, 1] == fin.sum(), (what, r)
        assert abs(per["q_sum"][r, 0] - q[fin].sum()) <= 1e-12 * N, (what, r)
    assert per["hb_hist"].sum() == 3 * R * N
    # summed outputs, and identical bits from call to call
    assert np.array_equal(tot["hb_hist"], per["hb_hist"].sum(0)), what
    assert np.array_equal(tot["q_hist"], per["q_hist"].sum(0)), what
    assert np.array_equal(tot["q_sum"].view(np.uint64), per["q_sum"].view(np.uint64)), what
    again = b.local_order(q_bins, r_hb, theta, per_replica=True, details=True)
    for k in per:
        assert np.array_equal(per[k].view(np.uint8), again[k].view(np.uint8)), (what, k)
    return per, tot


def small_system(n_mol, box, seed):
    return common.random_system(n_mol, box, seed=seed, na_choices=(3,))


@pytest.mark.parametrize("n_mol", [5, 6, 64, 65, 129])
def test_small_and_odd_systems(n_mol):
    """The minimum of five, one lane pass (64), a second pass with one molecule (65), three passes
    (129); mixed atom types, so the SoA arrays are read.  r_hb = 7 and 11 (half the box) make
    dozens of candidates per molecule: counts clamp, and at 129 molecules a candidate list passes
    64 entries inside the scan."""
    box = 22.0
    a = small_system(n_mol, box, seed=300 + n_mol)
    with make_batch(a, 3) as b:
        for r in (1, 2):                                       # replicas differ
            sh = np.random.default_rng(r).random(3) * box
            b.set_replica(r, (a["com"] + sh) % box, a["coords"] + np.repeat((a["com"] + sh) % box - a["com"], 3, axis=0))
        b.recip_long()
        check_batch(b, [box] * 3, what=f"n_mol {n_mol}")
        per, _ = check_batch(b, [box] * 3, q_bins=7, r_hb=7.0, theta=50.0, what=f"n_mol {n_mol}, r_hb 7")
        check_batch(b, [box] * 3, q_bins=4096, r_hb=11.0, theta=75.0, what=f"n_mol {n_mol}, r_hb L/2")
        if n_mol >= 64:
            assert per["hb"].max() >= 2
        b.set_option("local_stage", 0)                         # the positions read from device memory
        check_batch(b, [box] * 3, what=f"n_mol {n_mol}, unstaged")
        check_batch(b, [box] * 3, q_bins=33, r_hb=11.0, theta=75.0, what=f"n_mol {n_mol}, unstaged, r_hb L/2")


def test_four_molecules_are_refused():
    a = small_system(4, 22.0, seed=7)
    with make_batch(a, 2) as b:
        out = sentinels(b, 10)
        with pytest.raises(_lib.MMCError) as ei:
            b.local_order(10, details=True, out=out)
        assert ei.value.status == _lib.MMC_ERR_UNSUPPORTED
        assert untouched(out)


@pytest.mark.parametrize("variant", ["unwrapped", "reference"])
def test_nist_config_1_in_both_com_conventions(variant):
    a = common.nist_arrays(1, variant)
    with make_batch(a, 3) as b:
        b.run(150, T, 0.4, 0.2, seed=2, n_groups=1)            # replicas diverge
        per, tot = check_batch(b, [a["box"]] * 3, what=variant)
        assert not np.array_equal(per["nbr"][0], per["nbr"][1])
        assert tot["hb_hist"][0, 1:].sum() > 0                  # water: bonds are there
        assert np.array_equal(tot["hb_hist"][0] @ np.arange(9), tot["hb_hist"][1] @ np.arange(9))  # nothing clamps
        b.set_option("local_stage", 0)
        check_batch(b, [a["box"]] * 3, q_bins=100, what=variant + ", unstaged")


def test_750_molecules():
    a = common.nist_arrays(4, "unwrapped")
    with make_batch(a, 3) as b:
        b.set_option("device_moves", 1)
        b.run(300, T, DR, DPHI, seed=4242)
        per, tot = check_batch(b, [a["box"]] * 3, what="cfg4")
        from metropolismontecarlo_amd import observables as obs
        n_hb = obs.hbonds_per_molecule(tot["hb_hist"])
        assert 1.5 < n_hb[2] < 4.5 and n_hb[0] == n_hb[1]       # water at 0.83 g/cm^3; nothing clamps
        assert 0.2 < obs.tetrahedral_mean(tot["q_sum"].sum(0)) < 0.9
        check_batch(b, [a["box"]] * 3, q_bins=4096, r_hb=3.2, theta=20.0, what="cfg4, one wave per workgroup")


def lattice_arrays(n, spacing):
    """A simple-cubic lattice of waters with the force field of NIST configuration 1."""
    a = common.nist_arrays(1, "unwrapped")
    O, box = ref.cubic_lattice(n, spacing)
    coords = ref.frame(O, box)
    m = len(O)
    w = np.array([15.9994, 1.008, 1.008])
    com = (coords.reshape(m, 3, 3) * w[None, :, None]).sum(1) / w.sum()
    return dict(a, com=com, coords=coords, atype=np.tile(a["atype"][:3], m), charge=np.tile(a["charge"][:3], m),
                box=float(box))


@pytest.mark.parametrize("n,spacing", [(4, 5.5), (5, 4.5)])
def test_lattice_ties_go_to_the_lower_index(n, spacing):
    """Six neighbours at bit-equal r^2: in 64 different lanes (n = 4), and two passes of the lanes so
    that equal keys also meet inside a lane (n = 5)."""
    a = lattice_arrays(n, spacing)
    with make_batch(a, 2) as b:
        per, _ = check_batch(b, [a["box"]] * 2, r_hb=spacing + 0.5, what=f"lattice {n}")
        d, r2 = ref.oo_vectors(a["coords"], a["box"])
        for i in range(n ** 3):
            assert list(per["nbr"][0, i]) == sorted(np.flatnonzero(r2[i] == spacing * spacing))[:4], i
        b.set_option("local_stage", 0)
        check_batch(b, [a["box"]] * 2, r_hb=spacing + 0.5, what=f"lattice {n}, unstaged")


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
        check_batch(b, boxes, q_bins=50, what="per box, after sweeps")
        check_batch(b, boxes, q_bins=50, r_hb=0.5 * boxes.min(), theta=10.0, what="per box, half the smallest box")
        out = sentinels(b, 50)
        with pytest.raises(_lib.MMCError) as ei:
            b.local_order(50, r_hb=np.nextafter(0.5 * boxes.min(), 100.0), details=True, out=out)
        assert ei.value.status == _lib.MMC_ERR_ARG and untouched(out)


@pytest.mark.parametrize("system", ["records", "arrays"])
def test_launch_shape_does_not_change_the_results(system):
    n_cus = common.device_cu_count()
    R = 10 * n_cus + 1                                      # 2.5 replicas per workgroup of the default grid
    a = common.nist_arrays(1, "unwrapped") if system == "records" else small_system(65, 22.0, seed=17)
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
        base_per, base_tot = check_batch(b, boxes, q_bins=64, replicas=some, what=system)
        if system == "records":
            assert not np.array_equal(base_per["nbr"][0], base_per["nbr"][R - 1])
        for wgs, stage in ((1, 1), (3, 1), (0, 0), (1, 0)):
            b.set_option("wave_wgs", wgs)
            b.set_option("local_stage", stage)
            per = b.local_order(64, per_replica=True, details=True)
            tot = b.local_order(64)
            for k in base_per:
                assert np.array_equal(per[k].view(np.uint8), base_per[k].view(np.uint8)), (system, wgs, stage, k)
            for k in base_tot:
                assert np.array_equal(tot[k].view(np.uint8), base_tot[k].view(np.uint8)), (system, wgs, stage, k)
        b.set_option("wave_wgs", 0)
        b.set_option("local_stage", 1)


def chain(b, interleave, n_blocks=2, steps=60):
    e = b.potential_ewald(as_array=True)["energy"].copy()
    stats = []
    for blk in range(n_blocks):
        e, st = b.run(steps, T, DR, DPHI, seed=21, energies=e)
        stats.append({k: v for k, v in st.items() if isinstance(v, int)})
        if interleave:
            b.local_order(50, per_replica=bool(blk & 1), details=bool(blk & 1))
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


def test_wolf_style():
    a = common.nist_arrays(1, "unwrapped")
    with make_batch(a, 3) as b:
        b.set_option("device_moves", 1)
        b.set_coulomb_style("wolf")
        e = b.potential_wolf(as_array=True)["energy"].copy()
        b.run(90, T, 0.4, 0.2, seed=8, energies=e)
        per, _ = check_batch(b, [a["box"]] * 3, what="wolf")
        assert not np.array_equal(per["q"][0], per["q"][1])


def sentinels(b, q_bins, per_replica=False):
    R, N = b.R, b.n_mol
    lead = (R,) if per_replica else ()
    return dict(hb_hist=np.full(lead + (3, 9), 99, dtype=np.uint64), q_hist=np.full(lead + (max(q_bins, 0),), 99, dtype=np.uint64),
                q_sum=np.full((R, 2), 7.5), nbr=np.full((R, N, 4), -5, dtype=np.int32), q=np.full((R, N), 7.5),
                hb=np.full((R, N, 2), 99, dtype=np.uint8))


def untouched(out):
    return (np.all(out["hb_hist"] == 99) and np.all(out["q_hist"] == 99) and np.all(out["q_sum"] == 7.5)
            and np.all(out["nbr"] == -5) and np.all(out["q"] == 7.5) and np.all(out["hb"] == 99))


def test_refusals_leave_outputs_untouched():
    a = common.nist_arrays(1, "unwrapped")
    R = 2
    L = _lib.lib()

    def expect(status, b, q_bins=10, per=False, **kw):
        out = sentinels(b, q_bins, per)
        with pytest.raises(_lib.MMCError) as ei:
            b.local_order(q_bins, per_replica=per, details=True, out=out, **kw)
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
            expect(_lib.MMC_ERR_ARG, b, r_hb=r_hb, per=True)
        for theta in (120.0, 180.0, float("nan")):             # cos_hb <= 0 or NaN (cos 90 deg rounds to 6e-17 > 0) ...
            expect(_lib.MMC_ERR_ARG, b, theta_deg=theta)
        hb = np.full((3, 9), 99, dtype=np.uint64)
        p64 = hb.ctypes.data_as(_lib.C.POINTER(_lib.C.c_uint64))
        for cos_hb in (0.0, -0.2, np.nextafter(1.0, 2.0), float("nan")):   # ... so cos_hb itself through the C call
            assert L.mmc_batch_local_order(b._h, 3.5, cos_hb, 10, 0, p64, None, None, None, None, None) == _lib.MMC_ERR_ARG
        for nb in (0, -3, 4097):
            assert L.mmc_batch_local_order(b._h, 3.5, 0.8, nb, 0, p64, None, None, None, None, None) == _lib.MMC_ERR_ARG
        assert L.mmc_batch_local_order(b._h, 3.5, 0.8, 10, 0, None, None, None, None, None, None) == _lib.MMC_ERR_ARG
        assert np.all(hb == 99)
        expect(_lib.MMC_ERR_ARG, b, q_bins=4097)
        # ... and after all that the call works, r_hb = L / 2 and cos_hb = 1 exactly included, with one output only
        assert L.mmc_batch_local_order(b._h, a["box"] / 2, 1.0, 10, 0, p64, None, None, None, None, None) == _lib.MMC_OK
        assert hb[0].sum() == hb[1].sum() == hb[2].sum() == R * b.n_mol
        assert np.array_equal(b.local_order(10)["hb_hist"].sum(1), hb.sum(1))
    # a volume trial in flight
    with per_box_batch(per_box_states([1.0, 1.02])) as b:
        boxes = b.get_boxes()
        b.volume_trial_replicas(boxes * np.array([1.01, 0.0]))
        expect(_lib.MMC_ERR_STATE, b)
        b.volume_settle(np.zeros(R, dtype=np.int32))
        assert b.local_order(10)["q_hist"].sum() == R * b.n_mol
