"""Wolf-style chains (mmc_batch_set_coulomb_style) on every path the move kernels' WOLF
instantiations branch on, against the oracle -- what test_gpu_replay_paths.py, the
several-steps-per-launch / long-list tests of test_gpu_batch.py and test_gpu_whole_call.py are to
the Ewald chain: IMG = false with device-made moves, the quaternion routes behind the Wolf-only
commit fence, more parts than molecules (np = n_parts), several units per wave and the ticket
queue at 2, 4, 8 and 16 steps per launch, whole_call, the default launch cap (WV_OCC_WOLF), the
generic kernel on mixtures, the neighbour-list flush, the (sum q)^2 term of the Wolf total,
host-made proposals through run, bit-identity across deciders and layouts, and the observers.

One replay: test_gpu_replay_paths.replay(wolf=True) -- dU = d_lj + d_real, the oracle's S arrays
left alone.  Tolerances are the project's: TOL (|dU| + 1e4) per step, the flag byte exact, 2e-13 A
on coordinates, 4e-16 per accepted rotation on quaternions, TOL 1e5 on a call's energy change and
on running total against recompute, rel < TOL on potential_wolf's fields, view(np.uint64) where a
test says bit for bit.

Every run goes through run_wolf(), which asserts the move count and that no step went through the
move server (server_steps == 0) and records sum_old of the replicas to check before the run; every
test then calls check_state() -- directly, or through check_chain() where there is a replay -- for
those replicas: get_replica's sum_old bitwise what it was before the run, the running total against
the recompute, and potential_wolf of the final state against orc.potential_wolf of the downloaded
coordinates.

The scenario functions at the top (seeds, systems, replays) touch no GPU: tests/
test_wolf_paths_host.py asserts their preconditions in the suite that runs without one."""
import functools
import math

import numpy as np
import pytest

import common
import structure_ref as ref
import test_gpu_replay_paths as rp
from common import rel
from test_gpu_replay_paths import (M_DPHI, M_DR, M_RCUT, M_STEPS, M_T, Q_DPHI, Q_DR, Q_RCUT, Q_STEPS, Q_T,
                                   T_DPHI, T_DR, T_RCUT, T_STEPS, T_T, TINY, W_DPHI, W_DR, W_RCUT, W_STEPS, W_T,
                                   make_batch, system)
from test_gpu_wolf import check_totals, oracle_ewald

pytestmark = pytest.mark.gpu

TOL = 1e-9
CHECK = (0, 3, 4, 7)                        # both ends of both groups of eight replicas
COUNTS = ("moves", "trans_attempt", "trans_accept", "rot_attempt", "rot_accept", "overlaps")


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


# ---- scenarios (no GPU) ----------------------------------------------------------------------------
def wreplay(name, faithful, replica, calls, T, dr, dphi, rcut, probe=False):
    """The cached Wolf replay of a named system of test_gpu_replay_paths.system()."""
    return rp.replay_of(name, faithful, replica, tuple(calls), T, dr, dphi, rcut, probe, True)


@functools.lru_cache(maxsize=None)
def q216_straddling():
    """The 216-molecule equivalent of NIST configuration 4's "reference" variant (io.nist_system):
    every atom of q216 wrapped into [0, L) on its own and the centre of mass taken as the
    mass-weighted mean of those raw atoms (ReadNIST, quirk Q11), so a molecule that straddles the
    boundary has its COM near the middle of the box and atoms ~L / 2 from it: gate + 2 r_mol < L / 2
    fails on its own and the launch takes IMG = false whatever option image_by_molecule says."""
    a = system("q216", False)[0]
    box = a["box"]
    coords = a["coords"] - box * np.floor(a["coords"] / box)
    m = np.array([15.9994, 1.008, 1.008])                    # the masses of system()'s centres of mass
    com = (coords.reshape(-1, 3, 3) * m[None, :, None]).sum(1) / m.sum()
    return dict(a, com=com, coords=coords)


def r_mol_max(a):
    return np.linalg.norm(a["coords"] - np.repeat(a["com"], 3, axis=0), axis=1).max()


@functools.lru_cache(maxsize=None)
def replay_arrays(key, replica, calls, T, dr, dphi, rcut):
    """The cached Wolf replay of rigid moves on a system that is not one of system()'s: key =
    "straddling", ("mix", order) or ("charged",)."""
    from oracle import oracle as orc
    a = q216_straddling() if key == "straddling" else mixture(*key[1:]) if key[0] == "mix" else charged_mixture()
    return rp.replay(orc, a, replica, [(n, s, 0) for n, s in calls], T, dr, dphi, rcut, wolf=True)


@functools.lru_cache(maxsize=None)
def mixture(order):
    return common.spce_tip3p_mixture(1, order)[0]


@functools.lru_cache(maxsize=None)
def charged_mixture():
    """The "blocks" mixture with a net charge.  Scaling all three charges of a TIP3P molecule leaves
    it neutral, so it is the TIP3P OXYGEN charges that are scaled by 1.1: every TIP3P molecule
    carries -0.0834 e and sum q = -4.17 e, the case in which potential_wolf's
    (sum q)^2 erfc(kappa r_c) / r_c is not multiplied by zero."""
    a, sp = common.spce_tip3p_mixture(1, "blocks")
    q = a["charge"].copy().reshape(-1, 3)
    q[sp == 1, 0] *= 1.1
    return dict(a, charge=q.ravel())


def charged_self_margin(orc):
    """(|self with the (sum q)^2 term - self without it|, |self|) of the charged mixture, the term
    taken from its definition (energy.jl:924-930) and `self` from the oracle."""
    a = charged_mixture()
    ew = oracle_ewald(orc, a)
    t = orc.potential_wolf(common.oracle_system(a), ew, M_RCUT, M_RCUT, literal_prefactor=False)
    sq = a["charge"].sum()
    term = sq * sq * math.erfc(ew.kappa * M_RCUT) / M_RCUT * ew.factor
    return term, abs(t["self"])


Q_SEED, Q_REPLICA0 = 31337, 11
TINY_SEED0, TINY_REPLICA0 = 2024, 7
MIX_SEED = 2718
W_SEED, W_R = 5150, 48
QM_R, QM_SEED, QM_REPLICA0 = 24, 4242, 3        # quaternion routes at several steps per launch
T8_R, T8_SEED, T8_STEPS = 8, 555, 61            # tiny17 / tiny18 at eight steps per launch
TQ_SEED0, TQ_REPLICA0 = 99, 21                  # mode 1 at one and two molecules
SWITCH_R, SWITCH_SEEDS = 16, (606, 707)         # mode 1, then the rigid generator, in the window
CHARGED_STEPS, CHARGED_SEED = 60, 1234


def quat_replays(mode):
    return {r: wreplay("q216", mode == 1, Q_REPLICA0 + r, ((Q_STEPS, Q_SEED, mode),), Q_T, Q_DR, Q_DPHI, Q_RCUT)
            for r in CHECK}


def window_replays():
    return {r: wreplay("window", True, r, ((W_STEPS, W_SEED, 1),), W_T, W_DR, W_DPHI, W_RCUT, probe=True)
            for r in range(W_R)}


def tiny_replays(n_mol):
    """Four replicas of tinyN.  (One molecule: every Wolf dU is exactly 0 -- no partner, no
    reciprocal part -- so every step is accepted at any temperature.)"""
    return {r: wreplay(f"tiny{n_mol}", False, TINY_REPLICA0 + r, ((T_STEPS, TINY_SEED0 + n_mol, 0),), T_T, T_DR,
                       T_DPHI, T_RCUT) for r in range(4)}


def mixture_replays(order):
    return {r: replay_arrays(("mix", order), r, ((M_STEPS, MIX_SEED),), M_T, M_DR, M_DPHI, M_RCUT) for r in CHECK}


def species_counts(order, o):
    """[(accepted, rejected) of species 0, of species 1] of one mixture chain."""
    sp = common.spce_tip3p_mixture(1, order)[1]
    n_mol = sp.shape[0]
    out = []
    for species in (0, 1):
        acc = [o["trace"][k][1] & 1 for k in range(M_STEPS) if sp[k % n_mol] == species]
        out.append((sum(acc), len(acc) - sum(acc)))
    return out


L_RCUT = 12.4
LONG_SYSTEMS = ((1700, 0.033101144), (2000, 0.06))


@functools.lru_cache(maxsize=None)
def dense_water(n_mol, rho):
    from test_gpu_batch import _dense_water
    return _dense_water(n_mol, rho=rho)


@functools.lru_cache(maxsize=None)
def scripted_moves(n_mol, rho):
    """The six scripted moves of test_long_neighbour_lists_and_many_molecules on the oracle's chain
    in Wolf style (accepted: the even steps without overlap): [(mol, com_new, atoms_new, want
    (d_lj, d_real, d_vir without d_recip / 3), overlap, accepted, common.scan_flushes of the move)]."""
    from oracle import oracle as orc
    a = dense_water(n_mol, rho)
    s = common.oracle_system(a)
    ew = oracle_ewald(orc, a)
    orc.recip_long(ew, s.coords, s.charge, s.box)
    rng, out = np.random.default_rng(17), []
    for step in range(6):
        i = int(rng.integers(1, n_mol + 1)) if step != 3 else n_mol   # the last molecule too
        d = (rng.random(3) - 0.5) * 0.5
        c_new, a_new = s.com[i - 1] + d, s.coords[3 * (i - 1):3 * i] + d
        flush = common.scan_flushes(s.com, [s.com[i - 1], c_new], L_RCUT, a["box"], exclude=i - 1)
        do, ovo = orc.trial_move(i, s, ew, L_RCUT, L_RCUT, c_new, a_new)
        accept = (step % 2 == 0) and not ovo
        out.append((i, c_new.copy(), a_new.copy(), np.array([do[0], do[1], do[3] - do[2] / 3]), ovo, accept, flush))
        if accept:
            s.com[i - 1] = c_new
            s.coords[3 * (i - 1):3 * i] = a_new
    return out


# ---- running and checking --------------------------------------------------------------------------
def run_wolf(a, R, rcut, opts, runs, check, quat=None, db=None, trace=False, n_groups=2, n_parts=1, replica0=0,
             n_threads=2, n_streams=0, between=None):
    """One batch in Wolf style through the calls `runs` [(n_steps, seed, mode, T, dr, dphi)]:
    device-made moves unless `opts` say otherwise, orientations (re)set before a call as its mode
    says, `between(b, k)` called after call k.  S(k) is built before the switch, so that sum_old
    holds something a run could disturb."""
    with make_batch(a, R, rcut) as b:
        b.set_option("device_moves", 1)
        for k, v in opts.items():
            b.set_option(k, v)
        b.recip_long()
        b.set_coulomb_style("wolf")
        t0 = b.potential_wolf(as_array=True).copy()
        s_before = {r: b.get_replica(r)[2].copy() for r in check}
        e, mode_now, traces, stats = t0["energy"].copy(), 0, [], []
        for k, (n_steps, seed, mode, T, dr, dphi) in enumerate(runs):
            if mode != mode_now:
                if mode:
                    b.set_orientations(quat, db, faithful=mode == 1)
                else:
                    b.set_orientations(None, None)
                mode_now = mode
            if trace:
                b.set_option("trace_steps", n_steps)
            e, st = b.run(n_steps, T, dr, dphi, seed=seed, energies=e, n_groups=n_groups, n_parts=n_parts,
                          n_threads=n_threads, n_streams=n_streams, replica0=replica0)
            assert st["moves"] == R * n_steps and st["server_steps"] == 0, st
            stats.append(st)
            if trace:
                traces.append(b.get_trace(n_steps))
            if between:
                between(b, k)
        final = {r: b.get_replica(r) + ((b.get_orientations(r) if mode_now else None),) for r in check}
        t1 = b.potential_wolf(as_array=True).copy()
        assert b.coulomb_style == "wolf"
    return dict(t0=t0, e1=e, t1=t1, traces=traces, s_before=s_before, final=final, stats=stats)


def check_state(orc, a, out, r, rcut, at):
    """What every run test checks of a replica, with or without a replay: sum_old untouched, the
    running total against the recompute, potential_wolf of the final state against the oracle."""
    com, coords, S, _ = out["final"][r]
    assert np.array_equal(S.view(np.uint64), out["s_before"][r].view(np.uint64)), (at, r, "S(k) touched")
    assert abs(out["e1"][r] - out["t1"]["energy"][r]) < TOL * 1e5, (at, r, out["e1"][r], out["t1"]["energy"][r])
    check_totals(orc, a, com, coords, out["t1"][r], rcut, (at, r, "final"))


def check_chain(orc, a, o, out, r, rcut, at, call=None):
    """Local replica r of run_wolf's result against its replay `o`: with `call` the trace of that
    call (o's trace sliced by the caller), then the final state."""
    if call is not None:
        rp._check_trace(o, *out["traces"][call], r, at)
    com, coords, _, q = out["final"][r]
    assert np.abs(com - o["com"]).max() < 2e-13 and np.abs(coords - o["coords"]).max() < 2e-13, (at, r)
    if q is not None and o["quat"] is not None:
        err = np.abs(q - o["quat"]).max(1)
        assert (err < 4e-16 * np.maximum(o["n_qrot"], 1)).all(), (at, r, err.max(), o["n_qrot"].max())
    assert abs((out["e1"][r] - out["t0"]["energy"][r]) - o["e_acc"]) < TOL * 1e5, (at, r)
    check_state(orc, a, out, r, rcut, at)


def same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


# ---- 1: several steps per launch, several units per wave -------------------------------------------
MULTI_SEED, MULTI_REPLICA0 = 777, 3


@pytest.mark.parametrize("per_launch,R,wave_wgs,which,image", [
    pytest.param(2, 24, 1, "q216", -1, id="2-R24-wgs1"), pytest.param(4, 24, 1, "q216", -1, id="4-R24-wgs1"),
    pytest.param(8, 24, 1, "q216", -1, id="8-R24-wgs1"), pytest.param(8, 24, 2, "q216", -1, id="8-R24-wgs2"),
    pytest.param(16, 24, 1, "q216", -1, id="16-R24-wgs1"), pytest.param(16, 24, 2, "q216", -1, id="16-R24-wgs2"),
    pytest.param(8, 48, 1, "q216", -1, id="8-R48-wgs1"), pytest.param(8, 25, 1, "q216", -1, id="8-R25-wgs1"),
    # IMG = false, MULTI = true: the option turned off, and a system whose condition fails on its own
    pytest.param(8, 24, 1, "q216", 0, id="8-R24-wgs1-image_by_molecule0"),
    pytest.param(8, 24, 1, "straddling", -1, id="8-R24-wgs1-straddling"),
])
def test_several_steps_per_launch_stepped_by_the_oracle(per_launch, R, wave_wgs, which, image, orc):
    """216 molecules, the kernel decides, 2 / 4 / 8 / 16 steps per launch (41 steps at 16, else 90:
    the last launch is short), one or two workgroups per launch so that a wave runs 3, 2 and 1, 6,
    4 and 3 units: launch and decision counts; accept, overlap and rotation counts of ALL replicas
    against their replays; the replicas at the edges of the unit -> wave map step for step in the
    end -- final coordinates, the energy change, S(k) bitwise, totals."""
    a = system("q216", False)[0] if which == "q216" else q216_straddling()
    n_steps = 41 if per_launch == 16 else 90
    check = common.replicas_by_wave_position(R, 2, wave_wgs, occ=common.wolf_occ())
    opts = dict(kernel=2, persistent=0, accept_on_device=1, steps_per_launch=per_launch, wave_wgs=wave_wgs,
                image_by_molecule=image)
    out = run_wolf(a, R, Q_RCUT, opts, [(n_steps, MULTI_SEED, 0, Q_T, Q_DR, Q_DPHI)], list(check),
                   replica0=MULTI_REPLICA0)
    st = out["stats"][0]
    assert st["launches"] == 2 * -(-n_steps // per_launch) and st["device_decisions"] == R * n_steps, st

    def replay_r(r):
        calls = ((n_steps, MULTI_SEED, 0),)
        if which == "q216":
            return wreplay("q216", False, MULTI_REPLICA0 + r, calls, Q_T, Q_DR, Q_DPHI, Q_RCUT)
        return replay_arrays("straddling", MULTI_REPLICA0 + r, ((n_steps, MULTI_SEED),), Q_T, Q_DR, Q_DPHI, Q_RCUT)

    os_ = [replay_r(r) for r in range(R)]
    assert st["trans_accept"] + st["rot_accept"] == sum(o["n_acc"] for o in os_), st
    assert st["overlaps"] == sum(o["n_ovl"] for o in os_) and st["rot_attempt"] == sum(o["n_rot"] for o in os_), st
    for r in check:
        check_chain(orc, a, os_[r], out, r, Q_RCUT, (per_launch, R, wave_wgs, which, check[r]))
        assert 0 < os_[r]["n_acc"] < n_steps


# ---- 2: chains continue across calls, and whole_call -----------------------------------------------
def test_several_steps_per_launch_chains_continue_across_calls(orc):
    """Three calls of 42, 8 and 29 steps with three seeds at eight steps per launch, three units per
    wave: the Philox counter continues, the sweep restarts, every call's last launch is short."""
    a = system("q216", False)[0]
    R, calls = 24, ((42, 9001), (8, 77), (29, 123456789))
    check = common.replicas_by_wave_position(R, 2, wave_wgs=1, occ=common.wolf_occ())
    opts = dict(kernel=2, persistent=0, accept_on_device=1, steps_per_launch=8, wave_wgs=1)
    out = run_wolf(a, R, Q_RCUT, opts, [(n, s, 0, Q_T, Q_DR, Q_DPHI) for n, s in calls], list(check),
                   replica0=MULTI_REPLICA0)
    for (n, _), st in zip(calls, out["stats"]):
        assert st["device_decisions"] == R * n and st["launches"] == 2 * -(-n // 8), (n, st)
    for r in check:
        o = wreplay("q216", False, MULTI_REPLICA0 + r, [(n, s, 0) for n, s in calls], Q_T, Q_DR, Q_DPHI, Q_RCUT)
        check_chain(orc, a, o, out, r, Q_RCUT, ("three calls", check[r]))
        assert 0 < o["n_acc"] < sum(n for n, _ in calls)


def test_whole_call_runs_the_same_chains(orc):
    """Calls of 20, 7, 1 and 33 steps on 48 replicas, six units per wave, in launches of eight steps
    and with option whole_call (one launch per group for up to 32 steps): the six counts of every
    call, coordinates, sum_old and potential_wolf bit for bit, running energies to 1e-12 relative
    (the steps of a launch are summed in another grouping, test_gpu_whole_call.py); a few replicas
    of both forms against the oracle."""
    a = system("q216", False)[0]
    R, calls, seed = 48, (20, 7, 1, 33), 4242
    check = list(range(R))
    got = []
    for whole in (0, 1):
        opts = dict(kernel=2, persistent=0, accept_on_device=1, wave_wgs=1, whole_call=whole)
        out = run_wolf(a, R, Q_RCUT, opts, [(n, seed, 0, Q_T, Q_DR, Q_DPHI) for n in calls], check)
        for n, st in zip(calls, out["stats"]):
            assert st["launches"] == 2 * -(-n // (32 if whole else 8)) and st["device_decisions"] == R * n, (whole, n, st)
        for r in check:
            check_state(orc, a, out, r, Q_RCUT, ("whole_call", whole))
        got.append(out)
    e8, ew_ = got
    for sa, sb in zip(e8["stats"], ew_["stats"]):
        assert [sa[k] for k in COUNTS] == [sb[k] for k in COUNTS]
    for r in check:
        for x, y in zip(e8["final"][r][:3], ew_["final"][r][:3]):
            assert same_bits(x, y), r
    assert e8["t1"].tobytes() == ew_["t1"].tobytes()
    assert np.max(np.abs(e8["e1"] - ew_["e1"]) / np.abs(e8["e1"])) < 1e-12
    where = common.replicas_by_wave_position(R, 2, wave_wgs=1, occ=common.wolf_occ())
    for r in list(where)[:4]:
        o = wreplay("q216", False, r, [(n, seed, 0) for n in calls], Q_T, Q_DR, Q_DPHI, Q_RCUT)
        for out in got:
            check_chain(orc, a, o, out, r, Q_RCUT, ("whole_call", where[r]))
        assert 0 < o["n_acc"] < sum(calls)


# ---- 3: the default launch cap ---------------------------------------------------------------------
def test_default_launch_cap_stepped_by_the_oracle(orc):
    """Kernel 3 with the decision left to the library and no wave_wgs: the launch is capped at
    4 WV_OCC_WOLF / WV_MWAVES workgroups per compute unit (mmc_batch.inc).  R from the device's
    compute units so that each of the two groups has one and a half times 4 WV_OCC_WOLF n_cus
    units -- waves with two units and waves with one.  40 steps in launches of eight: every
    replica's running total against potential_wolf of the final state, replicas at the edges of the
    unit -> wave map against the oracle."""
    a = system("q216", False)[0]
    n_cus, occ, n_steps, seed = common.device_cu_count(), common.wolf_occ(), 40, 6061
    per_group = 4 * occ * n_cus
    per_group += per_group // 2 + 1
    R = 2 * per_group
    waves = common.wave_units(per_group, 0, n_cus, occ)
    assert per_group > 4 * occ * n_cus and max(len(w) for w in waves) >= 2 > min(len(w) for w in waves)
    check = common.replicas_by_wave_position(R, 2, 0, n_cus, occ=occ)
    out = run_wolf(a, R, Q_RCUT, dict(kernel=3, accept_on_device=-1), [(n_steps, seed, 0, Q_T, Q_DR, Q_DPHI)],
                   list(check), n_parts=0)
    st = out["stats"][0]
    assert st["device_decisions"] == R * n_steps and st["launches"] == 2 * -(-n_steps // 8), st
    worst = int(np.argmax(np.abs(out["e1"] - out["t1"]["energy"])))
    assert abs(out["e1"][worst] - out["t1"]["energy"][worst]) < TOL * 1e5, (worst, out["e1"][worst])
    for r in check:
        o = wreplay("q216", False, r, ((n_steps, seed, 0),), Q_T, Q_DR, Q_DPHI, Q_RCUT)
        check_chain(orc, a, o, out, r, Q_RCUT, ("default cap", check[r]))
        assert 0 < o["n_acc"] < n_steps


# ---- 4: one step per launch without the molecule image ---------------------------------------------
@pytest.mark.parametrize("parts", [1, 3])
def test_minimum_image_by_molecule_is_bit_identical(parts, orc):
    """216 molecules at r_cut 7 A pass gate + 2 r_mol < box / 2, so option image_by_molecule picks
    between the IMG = true and IMG = false Wolf instantiations (one part: <false, IMG, false, true>;
    three: <true, IMG, false, true>): traces, energies and accept counts bit for bit."""
    a = system("q216", False)[0]
    assert Q_RCUT + 2 * r_mol_max(a) + 1e-6 < a["box"] / 2
    R, n_steps, got = 24, 64, []
    for image in (-1, 0):
        out = run_wolf(a, R, Q_RCUT, dict(kernel=2, persistent=0, image_by_molecule=image),
                       [(n_steps, 99, 0, Q_T, Q_DR, Q_DPHI)], (0, R - 1), trace=True, n_parts=parts)
        got.append(out)
        for r in (0, R - 1):
            check_state(orc, a, out, r, Q_RCUT, (parts, image))
    x, y = got
    assert same_bits(x["traces"][0][0], y["traces"][0][0]) and np.array_equal(x["traces"][0][1], y["traces"][0][1])
    assert same_bits(x["e1"], y["e1"])
    acc = [o["stats"][0]["trans_accept"] + o["stats"][0]["rot_accept"] for o in got]
    assert acc[0] == acc[1] and 0 < acc[0] < R * n_steps


# ---- 5: quaternion routes --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("kernel,on_device,parts", [
    pytest.param(2, 0, 3, id="k2-host-3parts"), pytest.param(2, 1, 1, id="k2-device-1part"),
    pytest.param(1, 0, 2, id="k1-2parts"), pytest.param(0, 0, 0, id="k0")])
def test_quaternion_route_stepped_by_the_oracle(mode, kernel, on_device, parts, orc):
    """Modes 1 and 2 commit through quat_commit behind the Wolf-only fence of k_move_eval_wave:
    every step of the replicas at both ends of both groups, then coordinates, quaternions
    (get_orientations) and totals."""
    a, quat, db = system("q216", mode == 1)
    opts = dict(kernel=kernel, persistent=0, accept_on_device=on_device)
    out = run_wolf(a, 8, Q_RCUT, opts, [(Q_STEPS, Q_SEED, mode, Q_T, Q_DR, Q_DPHI)], CHECK, quat, db, trace=True,
                   n_parts=parts, replica0=Q_REPLICA0)
    assert out["stats"][0]["device_decisions"] == (8 * Q_STEPS if on_device else 0)
    os_ = quat_replays(mode)
    for r in CHECK:
        check_chain(orc, a, os_[r], out, r, Q_RCUT, (mode, kernel), call=0)
    assert sum(Q_STEPS - o["n_acc"] for o in os_.values()) > 20
    assert sum(int(o["n_qrot"].sum()) for o in os_.values()) > 100


@pytest.mark.parametrize("mode,per_launch", [(1, 8), (1, 16), (2, 8), (2, 16)])
def test_quaternion_route_several_steps_per_launch(mode, per_launch, orc):
    a, quat, db = system("q216", mode == 1)
    R, seed, replica0 = QM_R, QM_SEED, QM_REPLICA0
    check = common.replicas_by_wave_position(R, 2, wave_wgs=1, occ=common.wolf_occ())
    opts = dict(kernel=2, persistent=0, accept_on_device=1, steps_per_launch=per_launch, wave_wgs=1)
    out = run_wolf(a, R, Q_RCUT, opts, [(Q_STEPS, seed, mode, Q_T, Q_DR, Q_DPHI)], list(check), quat, db,
                   replica0=replica0)
    st = out["stats"][0]
    assert st["device_decisions"] == R * Q_STEPS and st["launches"] == 2 * -(-Q_STEPS // per_launch), st
    for r in check:
        o = wreplay("q216", mode == 1, replica0 + r, ((Q_STEPS, seed, mode),), Q_T, Q_DR, Q_DPHI, Q_RCUT)
        check_chain(orc, a, o, out, r, Q_RCUT, (mode, per_launch, check[r]))
        assert 0 < o["n_acc"] < Q_STEPS


def test_image_bound_window_against_the_oracle(orc):
    """Mode 1 in the window at 1e7 K: the Wolf replay's own chains must cross box / 2 in at least
    three replicas; the kernels must then take the per-atom image although the uploaded molecules
    pass the condition: every step and the final state of all 48 replicas."""
    a, quat, db = system("window", True)
    os_ = window_replays()
    hits = [r for r in range(W_R) if os_[r]["crossed"]]
    assert len(hits) >= 3, hits
    out = run_wolf(a, W_R, W_RCUT, dict(kernel=2, persistent=0, accept_on_device=0),
                   [(W_STEPS, W_SEED, 1, W_T, W_DR, W_DPHI)], range(W_R), quat, db, trace=True)
    for r in range(W_R):
        check_chain(orc, a, os_[r], out, r, W_RCUT, ("window", os_[r]["crossed"][:3]), call=0)


def test_mode_switch_keeps_the_bound(orc):
    """Mode 1 in the window, then the rigid generator on the deformed molecules: both calls' every
    step and the final state (the bound raised for mode 1 must outlive the mode)."""
    a, quat, db = system("window", True)
    R = SWITCH_R
    runs = [(W_STEPS, SWITCH_SEEDS[0], 1, W_T, W_DR, W_DPHI), (W_STEPS, SWITCH_SEEDS[1], 0, W_T, W_DR, W_DPHI)]
    out = run_wolf(a, R, W_RCUT, dict(kernel=2, persistent=0, accept_on_device=0), runs, range(R), quat, db,
                   trace=True)
    n_cross = 0
    for r in range(R):
        o = rp.replay(orc, a, r, [(W_STEPS, SWITCH_SEEDS[0], 1), (W_STEPS, SWITCH_SEEDS[1], 0)], W_T, W_DR, W_DPHI, W_RCUT, quat, db,
                      probe=True, wolf=True)
        n_cross += sum(1 for k in o["crossed"] if k >= W_STEPS)
        rp._check_trace(dict(o, trace=o["trace"][:W_STEPS]), *out["traces"][0], r, "mode 1")
        rp._check_trace(dict(o, trace=o["trace"][W_STEPS:]), *out["traces"][1], r, "rigid after mode 1")
        check_chain(orc, a, dict(o, quat=None), out, r, W_RCUT, "mode switch")
    assert n_cross > 0


# ---- 6: tiny systems -------------------------------------------------------------------------------
TINY_KERNELS = ((2, 0, 20, "k2-host-20parts"), (2, 1, 1, "k2-device"), (1, 0, 20, "k1-20parts"),
                (0, 0, 20, "k0-20parts"))


@pytest.mark.parametrize("n_mol,kernel,on_device,parts", [
    pytest.param(n, k, d, p, id=f"{n}-{name}") for n in TINY for k, d, p, name in TINY_KERNELS]
    + [pytest.param(17, 2, 0, 32, id="17-k2-host-32parts")])      # MMC_MAX_PARTS
def test_tiny_system_rigid_moves_stepped_by_the_oracle(n_mol, kernel, on_device, parts, orc):
    """With np = n_parts, 20 (and MMC_MAX_PARTS = 32) parts on 1-18 molecules leave most pair parts
    empty, at other indices than in Ewald style.  Every step against the oracle.  One molecule:
    every dU is exactly 0, every step accepted, so every step re-proposes a molecule whose commit
    is pending, and the final coordinates are the replay's only if each substitution was right."""
    a = system(f"tiny{n_mol}", False)[0]
    opts = dict(kernel=kernel, persistent=0, accept_on_device=on_device)
    out = run_wolf(a, 4, T_RCUT, opts, [(T_STEPS, TINY_SEED0 + n_mol, 0, T_T, T_DR, T_DPHI)], range(4), trace=True,
                   n_parts=parts, replica0=TINY_REPLICA0)
    assert out["stats"][0]["device_decisions"] == (4 * T_STEPS if on_device else 0)
    os_ = tiny_replays(n_mol)
    for r in range(4):
        check_chain(orc, a, os_[r], out, r, T_RCUT, (n_mol, kernel, parts), call=0)
    n_acc = sum(o["n_acc"] for o in os_.values())
    if n_mol == 1:
        d_gpu, f_gpu = out["traces"][0]
        assert (d_gpu == 0.0).all() and (f_gpu & 1).all() and n_acc == 4 * T_STEPS
        assert all(d == 0.0 for o in os_.values() for d, _ in o["trace"])
    else:
        assert n_acc > 20 and 4 * T_STEPS - n_acc > 5


@pytest.mark.parametrize("n_mol", [1, 2])
@pytest.mark.parametrize("on_device", [0, 1])
def test_tiny_system_quaternion_mode_stepped_by_the_oracle(n_mol, on_device, orc):
    """Mode 1 at one and two molecules: k_propose takes the pending record's q_new and coordinates,
    the wave kernel commits them behind the Wolf-only fence."""
    name = f"tiny{n_mol}"
    a, quat, db = system(name, True)
    R, seed, replica0 = 4, TQ_SEED0 + n_mol, TQ_REPLICA0
    out = run_wolf(a, R, T_RCUT, dict(kernel=2, persistent=0, accept_on_device=on_device),
                   [(T_STEPS, seed, 1, T_T, T_DR, T_DPHI)], range(R), quat, db, trace=True, replica0=replica0)
    n_sub = 0
    for r in range(R):
        o = wreplay(name, True, replica0 + r, ((T_STEPS, seed, 1),), T_T, T_DR, T_DPHI, T_RCUT)
        check_chain(orc, a, o, out, r, T_RCUT, (n_mol, on_device), call=0)
        f = [flags for _, flags in o["trace"]]
        n_sub += sum(1 for k in range(1, T_STEPS) if f[k - 1] & 1 and f[k] & 4)
    assert n_sub > 10        # accepted moves followed by a rotation of the molecule just committed


@pytest.mark.parametrize("n_mol", [17, 18])
def test_tiny_system_several_steps_per_launch(n_mol, orc):
    name = f"tiny{n_mol}"
    a = system(name, False)[0]
    R, seed, n_steps = T8_R, T8_SEED, T8_STEPS
    opts = dict(kernel=2, persistent=0, accept_on_device=1, steps_per_launch=8, wave_wgs=1)
    out = run_wolf(a, R, T_RCUT, opts, [(n_steps, seed, 0, T_T, T_DR, T_DPHI)], range(R))
    st = out["stats"][0]
    assert st["device_decisions"] == R * n_steps and st["launches"] == 2 * -(-n_steps // 8), st
    for r in range(R):
        o = wreplay(name, False, r, ((n_steps, seed, 0),), T_T, T_DR, T_DPHI, T_RCUT)
        check_chain(orc, a, o, out, r, T_RCUT, (n_mol, "K=8"))
        assert 0 < o["n_acc"] < n_steps


@pytest.mark.parametrize("kernel", [2, 1, 0])
def test_one_molecule_host_proposals(kernel, orc):
    """mmc_batch_eval at n_mol = 1 in Wolf style, four parts (three of them empty), three accept
    rules: d_recip == 0.0 exactly, the other terms against orc.trial_move, the settled state."""
    a = system("tiny1", False)[0]
    R, rng = 3, np.random.default_rng(5)
    rules = [lambda n: True, lambda n: False, lambda n: n % 3 != 1]
    s = [common.oracle_system(a) for _ in range(R)]
    ew = [oracle_ewald(orc, a) for _ in range(R)]
    for r in range(R):
        orc.recip_long(ew[r], s[r].coords, s[r].charge, a["box"])
    with make_batch(a, R, T_RCUT) as b:
        b.set_option("kernel", kernel)
        b.set_parts(4)
        b.recip_long()
        b.set_coulomb_style("wolf")
        s_before = [b.get_replica(r)[2].copy() for r in range(R)]
        acc_prev = np.zeros(R, dtype=bool)
        for n in range(24):
            shift = (rng.random(3) - 0.5) * 0.6
            com_new = np.array([s[r].com[0] + shift for r in range(R)])
            at_new = np.array([s[r].coords[:3] + shift for r in range(R)])
            if n % 2:     # a rotation about the centre of mass
                c, sn = math.cos(0.4 + n * 0.1), math.sin(0.4 + n * 0.1)
                Rz = np.array([[c, -sn, 0.0], [sn, c, 0.0], [0.0, 0.0, 1.0]])
                com_new = np.array([s[r].com[0] for r in range(R)])
                at_new = np.array([s[r].com[0] + (s[r].coords[:3] - s[r].com[0]) @ Rz.T for r in range(R)])
            d, ov = b.eval(1, com_new, at_new, acc_prev)
            for r in range(R):
                do, ovo = orc.trial_move(1, s[r], ew[r], T_RCUT, T_RCUT, com_new[r], at_new[r])
                want = np.array([do[0], do[1], do[3] - do[2] / 3])
                assert ov[r] == ovo and d[r][2] == 0.0, (n, r, d[r])
                assert np.abs(d[r][[0, 1, 3]] - want).max() < TOL * (np.abs(want).max() + 1e4), (n, r, d[r], want)
                acc_prev[r] = rules[r](n) and not ovo
                if acc_prev[r]:
                    s[r].com[0] = com_new[r]
                    s[r].coords[:3] = at_new[r]
        b.settle(acc_prev)
        tot = b.potential_wolf()
        for r in range(R):
            com, coords, S = b.get_replica(r)
            assert np.array_equal(com, s[r].com) and np.array_equal(coords, s[r].coords), r
            assert same_bits(S, s_before[r]), r
            check_totals(orc, a, com, coords, tot[r], T_RCUT, ("tiny1 eval", kernel, r))


@pytest.mark.parametrize("n_mol", TINY)
def test_tiny_system_totals(n_mol, orc):
    """potential_wolf of every tiny system at R = 1 and at R = 3 with distinct configurations."""
    a = system(f"tiny{n_mol}", False)[0]
    cases = [a, system(f"tiny{n_mol}", True)[0], dict(a, com=a["com"] + 0.37, coords=a["coords"] + 0.37)]
    with make_batch(a, 1, T_RCUT) as b:
        check_totals(orc, a, a["com"], a["coords"], b.potential_wolf()[0], T_RCUT, (n_mol, "R=1"))
    with make_batch(a, 3, T_RCUT) as b:
        for r, c in enumerate(cases):
            b.set_replica(r, c["com"], c["coords"])
        tot = b.potential_wolf()
        for r, c in enumerate(cases):
            check_totals(orc, a, c["com"], c["coords"], tot[r], T_RCUT, (n_mol, "R=3", r))


# ---- 7: mixtures on the generic kernel -------------------------------------------------------------
@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("order", common.MIX_ORDERS)
def test_mixture_stepped_by_the_oracle(order, parts, orc):
    """A mixture is not homogeneous, so the batch takes k_move_eval<true>: every step of the
    replicas at both ends of both groups; both species accepted and rejected in every chain."""
    a = mixture(order)
    out = run_wolf(a, 8, M_RCUT, dict(persistent=0, accept_on_device=0), [(M_STEPS, MIX_SEED, 0, M_T, M_DR, M_DPHI)],
                   CHECK, trace=True, n_parts=parts)
    assert out["stats"][0]["device_decisions"] == 0
    os_ = mixture_replays(order)
    for r in CHECK:
        check_chain(orc, a, os_[r], out, r, M_RCUT, (order, parts), call=0)
        assert all(acc > 0 and rej > 0 for acc, rej in species_counts(order, os_[r])), (order, r)


def test_charged_mixture_totals_and_chain(orc):
    """sum q != 0 (charged_mixture): potential_wolf's (sum q)^2 erfc(kappa r_c) / r_c against the
    oracle's literal double loop and its closed form, and a 60-step chain in which the constant
    must cancel: e1 - e0 against the oracle's sum of accepted dU."""
    a = charged_mixture()
    term, self_ = charged_self_margin(orc)
    assert term > 1e-6 * self_, (term, self_)
    moved = dict(a, com=a["com"].copy(), coords=a["coords"].copy())      # the TIP3P half displaced
    moved["com"][50:] += 0.21
    moved["coords"][150:] += 0.21
    cases = [a, dict(a, com=a["com"] + 0.37, coords=a["coords"] + 0.37), moved]
    with make_batch(a, 3, M_RCUT) as b:
        for r, c in enumerate(cases):
            b.set_replica(r, c["com"], c["coords"])
        tot = b.potential_wolf()
        for r, c in enumerate(cases):
            for literal in (True, False):
                to = orc.potential_wolf(common.oracle_system(c), oracle_ewald(orc, a), M_RCUT, M_RCUT,
                                        literal_prefactor=literal)
                for key in ("energy", "lj", "real", "self"):
                    assert rel(tot[r][key], to[key]) < TOL, (r, literal, key, tot[r][key], to[key])
    n_steps, seed = CHARGED_STEPS, CHARGED_SEED
    out = run_wolf(a, 8, M_RCUT, dict(persistent=0, accept_on_device=0), [(n_steps, seed, 0, M_T, M_DR, M_DPHI)],
                   CHECK, trace=True)
    for r in CHECK:
        o = replay_arrays(("charged",), r, ((n_steps, seed),), M_T, M_DR, M_DPHI, M_RCUT)
        check_chain(orc, a, o, out, r, M_RCUT, "charged", call=0)
        assert 0 < o["n_acc"] < n_steps


# ---- 8: long neighbour lists -----------------------------------------------------------------------
@pytest.mark.parametrize("kernel,parts,n_mol,rho", [
    pytest.param(k, p, n, rho, id=f"{k}-{p}" + ("" if n == 1700 else "-compressed"))
    for n, rho in LONG_SYSTEMS for k, p in ((2, 1), (1, 1), (2, 3), (1, 2))])
def test_long_neighbour_lists_and_many_molecules(kernel, parts, n_mol, rho, orc):
    """~250 (1700 molecules) and 430-520 (2000, compressed) neighbours inside the 12.4 A gate: the
    second neighbour tile and molecule chunk of k_move_eval_fast<true>, and at 2000 molecules the
    wave kernel's list is emptied mid-scan and process() called again, its sums adding up.  Six
    scripted moves against orc.trial_move and against a kernel-0 Wolf batch, then 60 steps with
    host-made and device-made proposals: the running total against potential_wolf."""
    a = dense_water(n_mol, rho)
    moves_ = scripted_moves(n_mol, rho)
    flushes = [m[6] for m in moves_]
    assert all(flushes) if n_mol == 2000 else not any(flushes), flushes
    with make_batch(a, 2, L_RCUT) as b, make_batch(a, 2, L_RCUT) as bg:
        for x, k, p in ((b, kernel, parts), (bg, 0, 1)):
            x.set_option("kernel", k)
            x.set_option("parts", p)
            x.recip_long()
            x.set_coulomb_style("wolf")
        s_before = b.get_replica(1)[2].copy()
        acc_prev = None
        for step, (i, c_new, a_new, want, ovo, accept, _) in enumerate(moves_):
            out, ov = b.eval(np.full(2, i), np.tile(c_new, (2, 1)), np.tile(a_new, (2, 1, 1)), accept_prev=acc_prev)
            outg, ovg = bg.eval(np.full(2, i), np.tile(c_new, (2, 1)), np.tile(a_new, (2, 1, 1)), accept_prev=acc_prev)
            scale = np.abs(want).max() + 1e4
            assert bool(ov[0]) == ovo == bool(ovg[0])
            assert out[0][2] == 0.0 and outg[0][2] == 0.0
            assert np.abs(out[0][[0, 1, 3]] - want).max() < TOL * scale, (step, out[0], want)
            assert np.abs(out[0] - outg[0]).max() < TOL * scale
            assert np.array_equal(out[0], out[1])
            acc_prev = np.full(2, accept)
        b.settle(acc_prev)
        bg.settle(acc_prev)
        for dev in (0, 1):
            b.set_option("device_moves", dev)
            t0 = b.potential_wolf(as_array=True)["energy"].copy()
            e1, st = b.run(60, 298.15, 0.3, 0.05, seed=3, energies=t0, n_groups=1, n_parts=parts)
            t1 = b.potential_wolf(as_array=True)
            assert np.abs(e1 - t1["energy"]).max() < 1e-9 * np.abs(t1["energy"]).max()
            assert st["trans_accept"] + st["rot_accept"] > 0 and st["server_steps"] == 0
        com, coords, S = b.get_replica(1)
        assert same_bits(S, s_before)
        check_totals(orc, a, com, coords, t1[1], L_RCUT, (kernel, parts, n_mol))


# ---- 9: host-made proposals through run ------------------------------------------------------------
@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("zero_copy", [0, 1])
@pytest.mark.parametrize("kernel", [2, 1, 0])
def test_host_made_proposals_through_run(kernel, zero_copy, parts, orc):
    """device_moves = 0: the host draws the moves, so the wave kernel runs <.., IMG = false, .., true>
    on records copied or read in place (zero_copy_moves).  Running total against potential_wolf of
    the final state, rigid molecules, accepted and rejected moves, S(k) bitwise."""
    a = system("q216", False)[0]
    R, n_steps = 6, 300
    opts = dict(device_moves=0, kernel=kernel, zero_copy_moves=zero_copy)
    out = run_wolf(a, R, Q_RCUT, opts, [(n_steps, 8128, 0, Q_T, Q_DR, Q_DPHI)], range(R), n_parts=parts)
    st = out["stats"][0]
    assert 0 < st["trans_accept"] + st["rot_accept"] < st["moves"] and st["device_decisions"] == 0, st

    def bonds(c):
        c = c.reshape(-1, 3, 3)
        return np.stack([np.linalg.norm(c[:, 0] - c[:, 1], axis=1), np.linalg.norm(c[:, 0] - c[:, 2], axis=1),
                         np.linalg.norm(c[:, 1] - c[:, 2], axis=1)])

    for r in range(R):
        check_state(orc, a, out, r, Q_RCUT, (kernel, zero_copy, parts))
        com, coords = out["final"][r][:2]
        assert np.abs(bonds(coords) - bonds(a["coords"])).max() < 1e-9
        assert (com >= 0).all() and (com <= a["box"]).all()
        assert np.abs(coords - a["coords"]).max() > 1e-3


# ---- 10: the same chains whoever decides and however laid out --------------------------------------
def test_deciders_give_the_same_chains(orc):
    """Host decision, kernel decision at one step per launch and at eight: final coordinates bit
    for bit and equal counts; every replica of every run through check_state."""
    a = system("q216", False)[0]
    R, n_steps, got = 24, 150, []
    for on_device, per_launch in ((0, 1), (1, 1), (1, 8)):
        opts = dict(kernel=2, persistent=0, accept_on_device=on_device, steps_per_launch=per_launch)
        out = run_wolf(a, R, Q_RCUT, opts, [(n_steps, 31, 0, Q_T, Q_DR, Q_DPHI)], range(R))
        st = out["stats"][0]
        assert st["device_decisions"] == (R * n_steps if on_device else 0)
        assert st["launches"] == 2 * -(-n_steps // per_launch), st
        for r in range(R):
            check_state(orc, a, out, r, Q_RCUT, ("decider", on_device, per_launch))
        got.append(out)
    for other in got[1:]:
        assert [got[0]["stats"][0][k] for k in COUNTS] == [other["stats"][0][k] for k in COUNTS]
        for r in range(R):
            assert all(same_bits(x, y) for x, y in zip(got[0]["final"][r][:3], other["final"][r][:3])), r
    acc = got[0]["stats"][0]["trans_accept"] + got[0]["stats"][0]["rot_accept"]
    assert 0 < acc < R * n_steps


def test_layout_does_not_change_the_chains(orc):
    """(groups, threads, streams): coordinates and energies bit for bit; every replica of every
    layout through check_state."""
    a = system("q216", False)[0]
    R, n_steps, got = 24, 150, []
    for groups, threads, streams in ((1, 1, 1), (2, 2, 2), (3, 2, 1)):
        out = run_wolf(a, R, Q_RCUT, dict(kernel=2, persistent=0), [(n_steps, 31, 0, Q_T, Q_DR, Q_DPHI)], range(R),
                       n_groups=groups, n_threads=threads, n_streams=streams)
        for r in range(R):
            check_state(orc, a, out, r, Q_RCUT, ("layout", groups, threads, streams))
        got.append(out)
    for other in got[1:]:
        assert same_bits(got[0]["e1"], other["e1"])
        assert [got[0]["stats"][0][k] for k in COUNTS] == [other["stats"][0][k] for k in COUNTS]
        for r in range(R):
            assert all(same_bits(x, y) for x, y in zip(got[0]["final"][r][:3], other["final"][r][:3])), r


# ---- 11: observers in Wolf style -------------------------------------------------------------------
def test_observers_between_calls_leave_the_chain_bit_identical(orc):
    """rdf, rdf_sites and dipoles are not fenced in Wolf style: called between three calls of 50
    steps they must leave coordinates and energies bit for bit, and give the histograms of
    tests/structure_ref.py and the dipoles of its fixed-order host sum on the batch's own state.
    Both batches' replicas through check_state."""
    a = system("q216", False)[0]
    R, numbins, seen = 6, 50, []

    def observe(b, k):
        per = b.rdf_sites(numbins, Q_RCUT, per_replica=True)
        tot = b.rdf_sites(numbins, Q_RCUT)
        one = b.rdf(0, numbins)
        d = b.dipoles()
        state = [b.get_replica(r) for r in range(R)]
        seen.append((per, tot, one, d, state))

    runs = [(50, 21, 0, Q_T, Q_DR, Q_DPHI)] * 3
    plain = run_wolf(a, R, Q_RCUT, {}, runs, range(R))
    watched = run_wolf(a, R, Q_RCUT, {}, runs, range(R), between=observe)
    for what, out in (("plain", plain), ("watched", watched)):
        for r in range(R):
            check_state(orc, a, out, r, Q_RCUT, ("observers", what))
    assert same_bits(plain["e1"], watched["e1"]) and plain["t1"].tobytes() == watched["t1"].tobytes()
    for r in range(R):
        assert all(same_bits(x, y) for x, y in zip(plain["final"][r][:3], watched["final"][r][:3])), r
    assert [[s[k] for k in COUNTS] for s in plain["stats"]] == [[s[k] for k in COUNTS] for s in watched["stats"]]
    box = a["box"]
    for per, tot, one, d, state in seen:
        want = np.stack([ref.six_rows(state[r][1], box, numbins, Q_RCUT) for r in range(R)])
        assert np.array_equal(per, want) and np.array_equal(tot, want.sum(0))
        full = np.stack([ref.six_rows(state[r][1], box, numbins, 0.0) for r in range(R)]).sum(0)
        assert np.array_equal(one, full[0])
        for r in range(R):
            mu = ref.molecule_dipoles(state[r][0], state[r][1], a["charge"], box)
            assert np.all(np.abs(d[r] - mu.sum(0)) <= 1e-12 * np.abs(mu).sum(0)), r
    assert not np.array_equal(seen[0][0], seen[-1][0])      # the chains moved between the calls
