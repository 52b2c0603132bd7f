"""Per-replica temperatures on every kernel form and run path that reads temps[r] and that
test_gpu_tempering.py leaves out.  (The eight k_move_eval_wave<false, IMG, MULTI, WOLF, LADDER = true>
forms against the oracle are rows of that file's PATHS table.)

1. The kernel's decisions against the host's, bit for bit, in all eight forms: NIST configuration 4
   "unwrapped" (IMG = true) and "reference" (IMG = false), Ewald and Wolf style, in launches of
   8 + 8 + 4, twenty of one step, 8 + 8 + 1 (a one-step launch closing a call of several-step ones)
   and one whole_call launch -- R = 24 in two groups at wave_wgs = 1, so a wave runs three units per
   launch (by fixed stride in the one-step form, by ticket in the others), and a temperature of its
   own for each of the 24 replicas, so that an index local to the group reads another's.
2. run_chains under a ladder: Driver::decide's per-chain bookkeeping behind temps[r], and the step
   size controller on each chain's own counters.
3. run_exchange on kernel 1, the move server, Wolf style and the one-step deciding kernel; its
   n_rounds = 0 and its refusal of per-replica boxes.

The scenario functions (seeds, ladders, replays) touch no GPU: tests/test_tempering_paths_host.py
asserts, in the suite that runs without one, that each ladder changes what it must.  Helpers,
constants and bounds are those of test_gpu_tempering.py, test_gpu_multi_record.py,
test_gpu_replay_paths.py and test_gpu_wolf_paths.py -- imported, not restated."""
import functools
import math

import numpy as np
import pytest

import common
import test_gpu_multi_record as mr
import test_gpu_replay_paths as rp
import test_gpu_tempering as tp
from common import rel
from metropolismontecarlo_amd import moves
from metropolismontecarlo_amd._lib import MMCError
from metropolismontecarlo_amd.structs import Moves
from test_gpu_replay_paths import Q_DPHI, Q_DR, Q_RCUT
from test_gpu_tempering import L_R, L_REPLICA0, L_SEED, L_STEPS, L_TEMPS, same_bits, same_states, state_of
from test_gpu_wolf_paths import COUNTS

pytestmark = pytest.mark.gpu


# ---- 1. device against host decisions in every form ------------------------------------------------
# Settled on the CPU with the oracle (test_tempering_paths_host.py asserts it).  With 24 rungs from
# 260 to 400 K and test_gpu_multi_record.py's seed, every (variant, style) has chains in both groups
# that the ladder changes, but none whose step 16 -- the lone last launch of 8 + 8 + 1 -- is decided
# otherwise at mr.T: its Metropolis uniforms fall outside every window [exp(-dU / T_r), exp(-dU / mr.T)],
# and a wider ladder (200-600, 150-800, 100-1200, 250-1000 K) does not move the uniforms.  So the
# ladder stays and the seed changes: of mr.SEED + 1, + 2, + 3 the second is the first that gives such
# a step in all four cases (replica 4, replica 17, or both).
D_SEED = mr.SEED + 2
D_TEMPS = moves.geometric_ladder(260.0, 400.0, mr.R)
D_CASES = [c for c in mr.CASES if mr.CASES[c][2] == mr.DR]           # both variants in both styles
D_SHORT = 2 * 8 + 1
D_GROUPS = 2
# shape: (options, steps, launches of the call)
SHAPES = {"8+8+4": (mr.ON_DEVICE, mr.N_STEPS, D_GROUPS * 3),
          "1x20": (dict(mr.ON_DEVICE, steps_per_launch=1), mr.N_STEPS, D_GROUPS * mr.N_STEPS),
          "8+8+1": (mr.ON_DEVICE, D_SHORT, D_GROUPS * 3),
          "whole": (dict(mr.ON_DEVICE, whole_call=1), mr.N_STEPS, D_GROUPS)}


def group_of(r):
    return r * D_GROUPS // mr.R


@functools.lru_cache(maxsize=None)
def nist4_replay(case, r, T):
    """Local replica r's mr.N_STEPS steps of the call at temperature T, stepped by the oracle (a
    call of D_SHORT steps is its beginning)."""
    from oracle import oracle as orc
    variant, style, dr = mr.CASES[case]
    a = common.nist_arrays(4, variant)
    return rp.replay(orc, a, mr.REPLICA0 + r, [(mr.N_STEPS, D_SEED, 0)], float(T), dr, mr.DPHI, mr.RCUT,
                     wolf=style == "wolf")


def accepts(o):
    return [f & 1 for _, f in o["trace"]]


def chains_the_ladder_changes(case):
    """Replicas whose accept trace at temps[r] is not their trace at mr.T, the scalar of the call."""
    return [r for r in range(mr.R)
            if accepts(nist4_replay(case, r, D_TEMPS[r])) != accepts(nist4_replay(case, r, mr.T))]


def chains_a_group_local_index_changes(case):
    """Replicas of the second group whose accept trace at temps[r] is not their trace at the
    temperature of the replica in their place in the first group."""
    half = mr.R // D_GROUPS
    return [r for r in range(half, mr.R)
            if accepts(nist4_replay(case, r, D_TEMPS[r])) != accepts(nist4_replay(case, r, D_TEMPS[r - half]))]


def last_launch_deciders(case):
    """Replicas whose step D_SHORT - 1, arrived at under temps[r], is decided one way at temps[r] and
    the other at mr.T: the same dU and overlap, the step's own Metropolis uniform (replay's rule)."""
    from test_gpu_moves import SLOT_METROPOLIS, philox_pair
    out, step = [], D_SHORT - 1
    for r in range(mr.R):
        delta, flags = nist4_replay(case, r, D_TEMPS[r])["trace"][step]
        u = philox_pair(D_SEED, mr.REPLICA0 + r, step, SLOT_METROPOLIS)[0]
        x = delta / mr.T
        at_scalar = (x < 0.0 or math.exp(-x) > u) and not flags & 2
        if int(at_scalar) != flags & 1:
            out.append(r)
    return out


@functools.lru_cache(maxsize=None)
def host_decisions(case, n_steps):
    variant, style, _ = mr.CASES[case]
    return tp._multi_record_run(common.nist_arrays(4, variant), mr.ON_HOST, D_TEMPS, style, n_steps, D_SEED)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("case", D_CASES)
def test_device_and_host_decide_alike_in_every_form(case, shape):
    """test_gpu_tempering.test_device_and_host_decide_alike_under_a_ladder over variant, style and
    launch shape: the six counts, every replica's centre of mass, coordinates and S(k) and the
    recomputed totals bit for bit, the running energies within test_gpu_multi_record.py's bounds,
    and the launch count of the shape."""
    variant, style, _ = mr.CASES[case]
    opts, n_steps, launches = SHAPES[shape]
    dev = tp._multi_record_run(common.nist_arrays(4, variant), opts, D_TEMPS, style, n_steps, D_SEED)
    tp.check_device_against_host(dev, host_decisions(case, n_steps), n_steps, launches, (case, shape))


# ---- 2. run_chains under a ladder ------------------------------------------------------------------
C_SCALAR = 555.0                                    # p->temperature of the calls: none of L_TEMPS
C_KW = dict(n_groups=2, n_parts=1, n_threads=2, replica0=L_REPLICA0)
C_SINGLE = 6


def chain_opts(on_device):
    return dict(kernel=2, persistent=0, accept_on_device=on_device, steps_per_launch=1)


@pytest.mark.parametrize("on_device", [1, 0])
def test_run_chains_is_run_under_a_ladder(on_device):
    """run_chains(adjust=False) on the chain of test_laddered_chains_stepped_by_the_oracle, the
    kernel deciding (one step per launch: the one-step LADDER form by another route) and the host:
    energies and final states are run's bit for bit -- run is pinned to the oracle there --, each
    chain's own counters are its replay's at temps[r], the running virial matches a recompute, and
    avg_energy / avg_virial add the running totals move by move."""
    a, _, _ = rp.system("q216", False)
    opts = chain_opts(on_device)
    with tp.open_batch(a, L_R, Q_RCUT, opts) as b:
        t0 = b.potential_ewald(as_array=True).copy()
        b.set_temperatures(L_TEMPS)
        e_run, st_run = b.run(L_STEPS, C_SCALAR, Q_DR, Q_DPHI, seed=L_SEED, energies=t0["energy"].copy(), **C_KW)
        fin_run = state_of(b)
    with tp.open_batch(a, L_R, Q_RCUT, opts) as b:
        b.potential_ewald()
        b.set_temperatures(L_TEMPS)
        ch = b.new_chains(t0["energy"], t0["virial"], dr_max=Q_DR, dphi_max=Q_DPHI)
        st = b.run_chains(ch, L_STEPS, C_SCALAR, seed=L_SEED, adjust=False, **C_KW)
        for s in (st, st_run):
            assert s["launches"] == 2 * L_STEPS and s["device_decisions"] == (L_R * L_STEPS if on_device else 0), s
        assert [st[k] for k in COUNTS] == [st_run[k] for k in COUNTS], (st, st_run)
        assert same_bits(ch["energy"], e_run) and same_states(state_of(b), fin_run)
        assert (ch["steps_taken"] == L_STEPS).all() and (ch["dr_max"] == Q_DR).all() and (ch["dphi_max"] == Q_DPHI).all()
        assert (ch["trans_attempt"] + ch["rot_attempt"] == L_STEPS).all()
        for r in range(L_R):
            o = tp.ladder_replay(r, L_TEMPS[r], False)
            assert ch["trans_naccept"][r] + ch["rot_naccept"][r] == o["n_acc"], r
            assert ch["rot_attempt"][r] == o["n_rot"] and ch["overlaps"][r] == o["n_ovl"], r
        t1 = b.potential_ewald(as_array=True).copy()
        for r in range(L_R):
            assert rel(ch["energy"][r], t1["energy"][r]) < rp.TOL, r
            assert rel(ch["virial"][r], t1["virial"][r]) < rp.TOL, r
        # averages.energy accumulates the running total after every move: one move at a time
        acc_e, acc_v = ch["avg_energy"].copy(), ch["avg_virial"].copy()
        for k in range(C_SINGLE):
            b.run_chains(ch, 1, C_SCALAR, seed=100 + k, adjust=False, **C_KW)
            acc_e += ch["energy"]
            acc_v += ch["virial"]
        assert same_bits(ch["avg_energy"], acc_e) and same_bits(ch["avg_virial"], acc_v)
        assert (ch["steps_taken"] == L_STEPS + C_SINGLE).all()


C_SWEEP = L_STEPS // 2                              # one sweep of the 216 molecules


def adjusted_step_sizes(counts, box):
    """(dr_max, dphi_max) after the host mirror of Adjust! / Adjust_rot! has seen `counts`, one
    (trans_naccept, trans_attempt, rot_naccept, rot_attempt) per sweep's end, from Q_DR and Q_DPHI."""
    mt, mq = Moves(0, 0, 0, 0, 0.5, Q_DR), Moves(0, 0, 0, 0, 0.5, Q_DPHI)
    for t_acc, t_att, q_acc, q_att in counts:
        mt.naccept, mt.attempt, mq.naccept, mq.attempt = int(t_acc), int(t_att), int(q_acc), int(q_att)
        moves.Adjust(mt, box)
        moves.Adjust_rot(mq, box)
    return mt, mq


def oracle_step_sizes(r):
    """What the controller makes of local replica r's two sweeps (two calls, seeds L_SEED and
    L_SEED + 1) as the oracle steps them at temps[r]."""
    o = rp.replay_of("q216", False, L_REPLICA0 + r, ((C_SWEEP, L_SEED, 0), (C_SWEEP, L_SEED + 1, 0)), float(L_TEMPS[r]),
                     Q_DR, Q_DPHI, Q_RCUT)
    flags = [f for _, f in o["trace"]]
    counts = [(sum(1 for f in flags[:n] if f & 5 == 1), sum(1 for f in flags[:n] if not f & 4),
               sum(1 for f in flags[:n] if f & 5 == 5), sum(1 for f in flags[:n] if f & 4))
              for n in (C_SWEEP, 2 * C_SWEEP)]
    mt, mq = adjusted_step_sizes(counts, rp.system("q216", False)[0]["box"])
    return mt.d_max, mq.d_max


def test_run_chains_adjusts_each_chain_by_its_own_counters():
    """run_chains(adjust=True), a sweep per call, twice: the controller fires at a sweep's end only,
    so each call's moves are run's with the step sizes the call began with -- energies and final
    states bit for bit -- and after each call every chain's dr_max and dphi_max are what the host
    mirror of Adjust! makes of that chain's own counters.  Two sweeps, because Adjust!'s first call
    only records (adjust.jl:3-5): the first leaves the step sizes alone, the second changes them,
    and the coldest and the hottest rung then hold different ones."""
    a, _, _ = rp.system("q216", False)
    opts = chain_opts(0)
    assert C_SWEEP == a["com"].shape[0]
    with tp.open_batch(a, L_R, Q_RCUT, opts) as b:
        t0 = b.potential_ewald(as_array=True).copy()
        b.set_temperatures(L_TEMPS)
        e_run = t0["energy"].copy()
        for sweep in range(2):
            e_run, _ = b.run(C_SWEEP, C_SCALAR, Q_DR, Q_DPHI, seed=L_SEED + sweep, energies=e_run, **C_KW)
        fin_run = state_of(b)
    with tp.open_batch(a, L_R, Q_RCUT, opts) as b:
        b.potential_ewald()
        b.set_temperatures(L_TEMPS)
        ch = b.new_chains(t0["energy"], t0["virial"], dr_max=Q_DR, dphi_max=Q_DPHI)
        counts = [[] for _ in range(L_R)]
        for sweep in range(2):
            st = b.run_chains(ch, C_SWEEP, C_SCALAR, seed=L_SEED + sweep, adjust=True, **C_KW)
            assert st["device_decisions"] == 0 and st["moves"] == L_R * C_SWEEP, st
            for r in range(L_R):
                counts[r].append(tuple(ch[k][r] for k in ("trans_naccept", "trans_attempt", "rot_naccept", "rot_attempt")))
                mt, mq = adjusted_step_sizes(counts[r], a["box"])
                assert ch["dr_max"][r] == mt.d_max and ch["dphi_max"][r] == mq.d_max, (sweep, r)
                assert ch["trans_attempp"][r] == mt.attempp and ch["rot_naccepp"][r] == mq.naccepp, (sweep, r)
            if sweep == 0:
                assert (ch["dr_max"] == Q_DR).all() and (ch["dphi_max"] == Q_DPHI).all()
        assert same_bits(ch["energy"], e_run) and same_states(state_of(b), fin_run)
        assert (ch["steps_taken"] == 2 * C_SWEEP).all()
        assert ch["dr_max"][0] != ch["dr_max"][L_R - 1], ch["dr_max"]
        for r in (0, L_R - 1):      # ... and they are what the oracle's chains at temps[r] give
            assert (ch["dr_max"][r], ch["dphi_max"][r]) == oracle_step_sizes(r), r


# ---- 3. run_exchange on the other deciding paths ---------------------------------------------------
# path: (options, n_parts, Wolf style) -- rows of test_gpu_tempering.PATHS
X_PATHS = {name: (tp.PATHS[row][0], tp.PATHS[row][1], tp.PATHS[row][3])
           for name, row in (("k1", "k1"), ("server", "server"), ("wolf-device-8", "wolf-device-8"),
                             ("wave-device-1", "wave-device-1-trace"))}


@pytest.mark.parametrize("path", list(X_PATHS))
def test_run_exchange_is_run_and_exchange_composed_on_every_path(path):
    """The composition of test_run_exchange_is_run_and_exchange_composed_by_hand -- run_exchange
    against run, set_temperatures and the pure exchange_round, bit for bit, swaps accepted and
    rejected -- with the host deciding on kernel 1's records, on the move server (started and
    released once per round, the temperatures uploaded in between), in Wolf style (the energies
    are the Wolf totals) and with the one-step deciding kernel."""
    opts, n_parts, wolf = X_PATHS[path]
    whole, st, t0, t1 = tp.exchange_whole(opts, n_parts, wolf)
    n_steps = tp.X_ROUNDS * tp.X_STEPS
    assert st["device_decisions"] == (st["moves"] if opts.get("accept_on_device") else 0), st
    assert st["server_steps"] == (n_steps if opts.get("persistent") == 1 else 0), st
    if opts.get("accept_on_device"):
        per_launch = opts["steps_per_launch"]
        assert st["launches"] == 2 * tp.X_ROUNDS * (tp.X_STEPS // per_launch), st
    hand, _ = tp.exchange_by_hand(tp.decide_pure, opts, n_parts, wolf)
    tp.check_exchange_composition(whole, hand, path)
    for r in range(tp.X_R):
        assert rel(whole["e"][r], t1["energy"][r]) < rp.TOL, (path, r)


def test_run_exchange_of_no_rounds_changes_nothing():
    a, _, _ = rp.system("q216", False)
    with tp.open_batch(a, tp.X_R, Q_RCUT, tp.DEVICE8) as b:
        e0 = b.potential_ewald(as_array=True)["energy"].copy()
        temps = np.tile(tp.X_LADDER, tp.X_R // tp.X_RUNGS)
        b.set_temperatures(temps)
        before, rung = state_of(b), moves.initial_rungs(tp.X_R, tp.X_RUNGS)
        e1, st, attempt, accept = b.run_exchange(0, tp.X_STEPS, Q_DR, Q_DPHI, tp.X_SEED, e0, rung, tp.X_RUNGS,
                                                 round0=tp.X_ROUND0, temperature=C_SCALAR, n_parts=1, **tp.X_KW)
        assert all(st[k] == 0 for k in COUNTS + ("launches", "device_decisions", "server_steps")), st
        assert not attempt.any() and not accept.any()
        assert same_bits(e1, e0) and same_states(state_of(b), before)
        assert np.array_equal(rung, moves.initial_rungs(tp.X_R, tp.X_RUNGS)) and np.array_equal(b.temperatures(), temps)
        assert same_bits(b.potential_ewald(as_array=True)["energy"], e0)


def test_run_exchange_refuses_per_replica_boxes():
    """mmc_batch_run_exchange on a batch with per-replica boxes: MMC_ERR_UNSUPPORTED before any
    move -- state, boxes, temperatures and rung as they were."""
    from test_gpu_npt_replicas import DPHI, DR, nist4_boxes, per_box_batch
    states = nist4_boxes((0.99, 0.99, 1.02, 1.02))
    temps = np.array([280.0, 350.0, 280.0, 350.0])
    with per_box_batch(states) as b:
        b.set_temperatures(temps)
        e0 = b.potential_ewald(as_array=True)["energy"].copy()
        before, boxes, rung = state_of(b), b.get_boxes(), moves.initial_rungs(4, 2)
        with pytest.raises(MMCError, match="MMC_ERR_UNSUPPORTED"):
            b.run_exchange(1, 4, DR, DPHI, 1, e0, rung, 2)
        assert same_states(state_of(b), before) and same_bits(b.get_boxes(), boxes)
        assert np.array_equal(b.temperatures(), temps) and rung.tolist() == [0, 1, 0, 1]
        assert same_bits(b.potential_ewald(as_array=True)["energy"], e0)
