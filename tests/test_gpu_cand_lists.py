"""Candidate lists of the move kernel's COM scan (csrc/mmc_cand.hpp; option "candidate_lists").

A step of k_move_eval_wave with one part per move may test only the chosen molecule's candidates
instead of every centre of mass, when a per-replica displacement bound proves that the list holds
every survivor of the prefilter.  The list the pair loops see is then the same in the same order, so
every GPU case here runs the same chains with the lists on and off and compares energies, counts,
coordinates and S(k) of every replica byte for byte; the counters of mmc_batch_cand_stats say which
path the steps took.  The CPU test restates the threshold arithmetic in numpy on random codes."""
import ctypes as C

import numpy as np
import pytest

import common

RCUT = 10.0
R = 24
T, DR, DPHI = 298.15, 0.316555789, 0.05
COUNTS = ("moves", "trans_attempt", "trans_accept", "rot_attempt", "rot_accept", "overlaps")


# ---- the threshold arithmetic, on the CPU -------------------------------------------------------------
def _dist2(a, b):
    """com_quant_dist2 in numpy: codes (..., 3) uint16; the wrapped signed 16-bit difference per axis."""
    d = (a.astype(np.int64) - b.astype(np.int64) + 32768) % 65536 - 32768
    return (d * d).sum(axis=-1)


def _lib_thresholds(gate, skin, box):
    from metropolismontecarlo_amd import _lib
    out = (C.c_uint32 * 3)()
    assert _lib.lib().mmc_cand_thresholds(gate, skin, box, out) == 0
    return int(out[0]), int(out[1]), int(out[2])


def _lib_within(a2, d2, budget):
    from metropolismontecarlo_amd import _lib
    a2 = np.ascontiguousarray(a2, dtype=np.uint32)
    d2 = np.ascontiguousarray(d2, dtype=np.uint32)
    out = np.zeros(a2.shape[0], dtype=np.uint8)
    u32p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    assert _lib.lib().mmc_cand_within(a2.shape[0], a2.ctypes.data_as(u32p), d2.ctypes.data_as(u32p), budget,
                                      out.ctypes.data_as(u8p)) == 0
    return out.astype(bool)


def test_wrapped_difference_is_the_cyclic_distance():
    a = np.array([[0, 0, 0], [65535, 1, 40000]], dtype=np.uint16)
    b = np.array([[32768, 0, 0], [1, 65535, 7232]], dtype=np.uint16)
    # the -32768 difference squares to 2^30; 65535 -> 1 is two units across the wrap; 40000 - 7232 = 32768
    assert _dist2(a, b).tolist() == [2 ** 30, 4 + 4 + 2 ** 30]


def test_within_is_never_optimistic_and_tight_to_a_unit():
    rng = np.random.default_rng(3)
    for budget in (1, 7, 4361, 65535):
        a = rng.integers(0, budget + 2, 4000)
        d = rng.integers(0, budget + 2, 4000)
        a2 = np.minimum(a * a + rng.integers(0, 3, 4000), 2 ** 32 - 1)  # (squares and their neighbours)
        d2 = np.minimum(d * d + rng.integers(0, 3, 4000), 2 ** 32 - 1)
        d2[:8] = 2 ** 32 - 1                                            # the stale mark never passes
        got = _lib_within(a2, d2, budget)
        for k in range(4000):
            x, y, b2 = int(a2[k]), int(d2[k]), budget * budget
            exact = x + y <= b2 and 4 * x * y <= (b2 - x - y) ** 2      # sqrt(x) + sqrt(y) <= budget, on integers
            assert not got[k] or exact, (budget, x, y)
            lo = (int(np.ceil(np.sqrt(x))) + int(np.ceil(np.sqrt(y))) + 1) <= budget
            assert got[k] or not lo, (budget, x, y)                     # a unit inside the budget always passes
        assert not got[:8].any()


@pytest.mark.parametrize("box,gate,skin", [(24.9, 11.2, 2.0), (24.9, 11.2, 0.5), (60.0, 9.0, 3.0)])
def test_every_prefilter_survivor_is_a_candidate(box, gate, skin):
    """Random code configurations q0, displacements up to the bound and across the wrap: whenever the
    step's test passes for a chosen molecule and its two states, every molecule within gate_q of
    either state is within t_build of the chosen molecule in the snapshot."""
    gate_q, t_build, budget = _lib_thresholds(gate, skin, box)
    assert 0 < budget < np.sqrt(t_build) - np.sqrt(gate_q) + 1
    rng = np.random.default_rng(int(box * 10 + skin * 100))
    n, passed, survivors = 600, 0, 0
    for trial in range(40):
        q0 = rng.integers(0, 65536, (n, 3)).astype(np.uint16)
        q0[:40] = rng.integers(-300, 300, (40, 3)).astype(np.int64).astype(np.uint16)  # a cluster across the wrap
        q0[40] = (q0[0].astype(np.int64) + 32768).astype(np.uint16)                       # the -32768 difference
        scale = rng.choice([0.2, 0.5, 0.9, 1.0]) * budget
        step = rng.normal(size=(n, 3))
        step *= (rng.random((n, 1)) * scale / np.linalg.norm(step, axis=1, keepdims=True))
        cur = (q0.astype(np.int64) + np.trunc(step).astype(np.int64)).astype(np.uint16)
        D = int(_dist2(cur, q0).max())
        for i in rng.integers(0, n, 30):
            move = np.trunc(rng.normal(size=3) * rng.random() * 0.4 * budget).astype(np.int64)
            states = np.stack([cur[i], (cur[i].astype(np.int64) + move).astype(np.uint16)])
            a2 = int(max(_dist2(states[0], q0[i]), _dist2(states[1], q0[i])))
            if not _lib_within([a2], [D], budget)[0]:
                continue
            passed += 1
            keep = (_dist2(cur, states[0]) < gate_q) | (_dist2(cur, states[1]) < gate_q)
            cand = _dist2(q0, q0[i]) < t_build
            survivors += int(keep.sum())
            assert not (keep & ~cand).any(), (trial, i)
    assert passed > 100 and survivors > passed  # (the chosen molecule itself survives, and it has neighbours)


# ---- the GPU cases ------------------------------------------------------------------------------------
def _batch(a, n_rep, lists, wave_wgs=1, rcut=RCUT, **options):
    from metropolismontecarlo_amd import structs
    from metropolismontecarlo_amd.device import Batch
    b = Batch(n_rep, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
              5.6 / a["box"], structs.factor, rcut, rcut)
    b.set_option("kernel", 2)
    b.set_option("persistent", 0)
    b.set_option("device_moves", 1)
    b.set_option("wave_wgs", wave_wgs)
    b.set_option("candidate_lists", lists)
    for k, v in options.items():
        b.set_option(k, v)
    return b


def _state(b, e, stats):
    return dict(e=np.array(e), counts=[[st[k] for k in COUNTS] for st in stats],
                reps=[b.get_replica(r) for r in range(b.R)], cand=b.cand_stats())


def _same(on, off):
    assert on["counts"] == off["counts"]
    assert on["e"].tobytes() == off["e"].tobytes()
    for r, (x, y) in enumerate(zip(on["reps"], off["reps"])):
        for u, v in zip(x, y):  # centres of mass, atoms, S(k)
            assert u.tobytes() == v.tobytes(), r
    assert off["cand"]["list_steps"] == 0 and off["cand"]["bytes"] == 0 and off["cand"]["state"] == 0


def _run(b, e, n, dr=DR, groups=2, **kw):
    return b.run(n, T, dr, DPHI, seed=97531, energies=e, n_groups=groups, n_parts=1, n_threads=2, **kw)


def _pair(scenario, a=None, n_rep=R, **kw):
    a = common.nist_arrays(4, "unwrapped") if a is None else a
    out = []
    for lists in (1, 0):
        with _batch(a, n_rep, lists, **kw) as b:
            out.append(scenario(b))
    _same(*out)
    return out[0]


BASIC = {  # wave_wgs, who decides / steps per launch, Coulomb style, COM variant, ladder
    "k8_img_wg1": dict(wave_wgs=1, accept_on_device=1, steps_per_launch=8),
    "k8_noimg_wg2": dict(wave_wgs=2, accept_on_device=1, steps_per_launch=8, image_by_molecule=0),
    "k1_host_wg1": dict(wave_wgs=1, accept_on_device=0),
    "k1_host_noimg_wg2": dict(wave_wgs=2, accept_on_device=0, image_by_molecule=0),
    "k8_wolf_wg2": dict(wave_wgs=2, accept_on_device=1, steps_per_launch=8),
    "k1_host_wolf_noimg_wg1": dict(wave_wgs=1, accept_on_device=0, image_by_molecule=0),
    "k8_ladder_wg2": dict(wave_wgs=2, accept_on_device=1, steps_per_launch=8),
    "k8_wolf_ladder_wg1": dict(wave_wgs=1, accept_on_device=1, steps_per_launch=8),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(BASIC))
def test_basic_paths(case):
    """Configuration 4, 24 replicas on one or two workgroups (a wave takes several units), two calls:
    every step takes a list -- within 53 steps a molecule moves at most once, by less than half the
    budget of a 2 A skin -- and the second call continues from the bound k_settle_rec left."""
    wolf, ladder = "wolf" in case, "ladder" in case

    def scenario(b):
        if wolf:
            b.set_coulomb_style("wolf")
        if ladder:
            b.set_temperatures(np.linspace(280.0, 340.0, b.R))
        e = (b.potential_wolf if wolf else b.potential_ewald)(as_array=True)["energy"].copy()
        stats = []
        for n in (40, 13):
            e, st = _run(b, e, n)
            assert st["server_steps"] == 0 and (st["device_decisions"] > 0) == ("k8" in case), st
            stats.append(st)
        return _state(b, e, stats)

    on = _pair(scenario, **BASIC[case])
    c = on["cand"]
    assert c["state"] == 1 and c["bytes"] > 2 * 256 * 750 * R and c["budget"] > 0
    assert c["list_steps"] == R * 53 and c["scan_steps"] == 0 and c["refreshes"] == R, c


@pytest.mark.gpu
def test_one_block():
    """27 molecules: one block, every molecule everyone's candidate (a skin that spans the box)."""
    from metropolismontecarlo_amd import io as mio
    box, com, coords = mio.cubic_lattice_water(27, 27 / 24.0 ** 3)
    ref = common.nist_arrays(4, "unwrapped")
    a = dict(com=com, coords=coords, box=box, atype=ref["atype"][:81], charge=ref["charge"][:81],
             eps=ref["eps"], sig=ref["sig"])

    def scenario(b):
        e = b.potential_ewald(as_array=True)["energy"].copy()
        stats = []
        for n in (40, 27):
            e, st = _run(b, e, n)
            stats.append(st)
        return _state(b, e, stats)

    on = _pair(scenario, a=a, rcut=6.0, wave_wgs=1, accept_on_device=1, steps_per_launch=8, cand_skin=15000)
    c = on["cand"]
    assert c["state"] == 1 and c["list_steps"] == R * 67 and c["scan_steps"] == 0, c


@pytest.mark.gpu
def test_overflow_falls_back():
    """A 4 A skin on configuration 4: every list is longer than its 256 slots, every step scans."""
    def scenario(b):
        e = b.potential_ewald(as_array=True)["energy"].copy()
        e, st = _run(b, e, 40)
        return _state(b, e, [st])

    on = _pair(scenario, wave_wgs=2, accept_on_device=1, steps_per_launch=8, cand_skin=4000)
    c = on["cand"]
    assert c["list_steps"] == 0 and c["scan_steps"] == R * 40 and c["refreshes"] == R, c


@pytest.mark.gpu
@pytest.mark.parametrize("calls", [(400,), (72, 8, 8, 40, 272)])
def test_bound_runs_out(calls):
    """dr_max = 2 A with a skin of 0.5 A (budget about 0.5 A).  A translation drawn from +-2 A per axis
    is almost always outside the budget itself and scans; rotations take the lists.  Of the 1.4 % of
    translations shorter than 0.6 A about a third are accepted, and one longer than three quarters of
    the budget makes its replica due: it scans until the rebuild the driver enqueues every eighth
    launch of a group.  9600 steps hold some dozens of those.  (With the default skin of 2 A the same
    step size never got a replica rebuilt in 19 200 steps: moves that long are not accepted.)  With
    several calls, calls end between a replica coming due and its rebuild."""
    def scenario(b):
        e = b.potential_ewald(as_array=True)["energy"].copy()
        stats = []
        for n in calls:
            e, st = _run(b, e, n, dr=2.0)
            stats.append(st)
        return _state(b, e, stats)

    on = _pair(scenario, wave_wgs=2, accept_on_device=1, steps_per_launch=8, cand_skin=500)
    c = on["cand"]
    print("bound runs out:", c, [x[2] for x in on["counts"]])
    assert c["list_steps"] + c["scan_steps"] == R * sum(calls)
    assert c["scan_steps"] > 0 and c["list_steps"] > 0 and c["refreshes"] > R, c


def _steps(b, e, n, stats, **kw):
    e, st = _run(b, e, n, **kw)
    stats.append(st)
    return e


@pytest.mark.gpu
def test_invalidation_by_reupload():
    def scenario(b):
        e = b.potential_ewald(as_array=True)["energy"].copy()
        stats = []
        e = _steps(b, e, 24, stats)
        com, coords, _ = b.get_replica(5)
        b.set_replica(3, com, coords)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        e = _steps(b, e, 24, stats)
        return _state(b, e, stats)

    c = _pair(scenario, wave_wgs=2, accept_on_device=1, steps_per_launch=8)["cand"]
    assert c["refreshes"] == 2 * R and c["list_steps"] == R * 48, c  # (every list rebuilt before the second call)


@pytest.mark.gpu
@pytest.mark.parametrize("between", ["fast_kernel", "generic_kernel", "server", "parts"])
def test_invalidation_by_another_kernel(between):
    """A run on a kernel that does not keep the bound, between two runs of the wave kernel."""
    def scenario(b):
        e = b.potential_ewald(as_array=True)["energy"].copy()
        stats = []
        e = _steps(b, e, 24, stats)
        if between == "server":
            b.set_option("persistent", 1)
            e = _steps(b, e, 16, stats)
            assert stats[-1]["server_steps"] == 16
            b.set_option("persistent", 0)
        elif between == "parts":  # (the wave kernel with the molecule range split: SUBST = true)
            e, st = b.run(16, T, DR, DPHI, seed=97531, energies=e, n_groups=2, n_parts=3, n_threads=2)
            stats.append(st)
        else:
            b.set_option("kernel", 1 if between == "fast_kernel" else 0)
            e = _steps(b, e, 16, stats)
            b.set_option("kernel", 2)
        before = b.cand_stats()
        e = _steps(b, e, 24, stats)
        after = b.cand_stats()
        assert after["refreshes"] - before["refreshes"] == (R if b.cand_stats()["state"] == 1 else 0)
        return _state(b, e, stats)

    c = _pair(scenario, wave_wgs=2, accept_on_device=1, steps_per_launch=8)["cand"]
    assert c["list_steps"] == R * 48 and c["scan_steps"] == 0, c


@pytest.mark.gpu
def test_invalidation_by_volume_moves():
    """mmc_batch_volume_trial / reject / accept (a one-replica batch held to the wave kernel): the codes
    are rewritten and restored, the thresholds change with the box."""
    def scenario(b):
        e = b.potential_ewald(as_array=True)["energy"].copy()
        stats = []
        e = _steps(b, e, 24, stats, groups=1)
        box = b.box
        b.volume_trial(box * 1.01, 5.6 / (box * 1.01))
        b.volume_reject()
        e = _steps(b, e, 24, stats, groups=1)
        b.volume_trial(box * 0.995, 5.6 / (box * 0.995))
        b.volume_accept()
        e = b.potential_ewald(as_array=True)["energy"].copy()
        e = _steps(b, e, 24, stats, groups=1)
        return _state(b, e, stats)

    c = _pair(scenario, n_rep=1, wave_wgs=1, accept_on_device=1, steps_per_launch=8)["cand"]
    assert c["refreshes"] == 3 and c["list_steps"] == 72, c


@pytest.mark.gpu
def test_invalidation_in_an_npt_chain():
    """mmc_batch_run_npt on a one-replica batch held to the wave kernel: sweeps of moves with a volume
    move after each, between two plain runs."""
    def scenario(b):
        e = b.potential_ewald(as_array=True)["energy"].copy()
        stats = []
        e = _steps(b, e, 40, stats, groups=1)
        e1, st, ns = b.run_npt(3, T, 1.0e-4, 300.0, DR, DPHI, 2468, float(e[0]), moves_per_sweep=24, n_parts=1, n_threads=1)
        assert ns["vol_attempt"] == 3
        stats.append(st)
        e = _steps(b, np.array([e1]), 40, stats, groups=1)
        s = _state(b, e, stats)
        s["box"] = b.box
        return s

    on = _pair(scenario, n_rep=1, wave_wgs=1)
    c = on["cand"]
    assert c["list_steps"] + c["scan_steps"] == 40 + 3 * 24 + 40 and c["refreshes"] >= 4, c
