"""Parallel tempering on the GPU: per-replica temperatures on every path that decides a move
(the wave kernel deciding itself in each of its eight LADDER forms -- molecule or per-atom image,
eight steps or one per launch, Ewald or Wolf style --, the wave kernel and kernels 0, 1 and 4 with
the host deciding, the move server, per-replica boxes and their volume criterion), the array
switched off again, and ladder exchanges through the batch against the pure function and its Python
restatement.  tests/test_gpu_tempering_paths.py goes on from here.

The chains are stepped by the oracle temperature by temperature: test_gpu_replay_paths.replay at
T = temps[r], with that file's tolerances (imported, not restated)."""
import functools
import math

import numpy as np
import pytest

import common
import tempering_ref
import test_gpu_multi_record as mr
import test_gpu_replay_paths as rp
from metropolismontecarlo_amd import moves
from metropolismontecarlo_amd._lib import MMCError
from metropolismontecarlo_amd.device import exchange_round
from test_gpu_replay_paths import Q_DPHI, Q_DR, Q_RCUT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.tobytes() == y.tobytes()


def same_states(fa, fb):
    return all(same_bits(x, y) for ra, rb in zip(fa, fb) for x, y in zip(ra, rb))


def state_of(b):
    return [b.get_replica(r) for r in range(b.R)]


DEVICE8 = dict(kernel=2, persistent=0, accept_on_device=1, steps_per_launch=8)


def open_batch(a, R, rcut, opts, wolf=False):
    b = rp.make_batch(a, R, rcut)
    b.set_option("device_moves", 1)
    for k, v in opts.items():
        b.set_option(k, v)
    if wolf:
        b.recip_long()
        b.set_coulomb_style("wolf")
    return b


# ---- 1. chains against the oracle, temperature by temperature ------------------------------------------
L_R, L_SEED, L_REPLICA0, L_STEPS = 8, 90210, 16, 2 * 216
L_TEMPS = moves.geometric_ladder(250.0, 1000.0, L_R)
L_SCALAR = 298.15                                   # p->temperature of the call: none of L_TEMPS
DEVICE1 = dict(DEVICE8, steps_per_launch=1)
PER_PAIR = dict(image_by_molecule=0)                 # the per-atom minimum image: IMG = false
HOST = dict(persistent=0, accept_on_device=0)
# path: (options, n_parts, traced, Wolf style, launches of the call).  The kernel's own decisions run
# k_move_eval_wave<false, IMG, MULTI, WOLF, LADDER = true>: IMG unless the path says PER_PAIR (216
# molecules at r_cut 7 A pass the molecule-image condition), MULTI where a launch takes eight steps
# -- one step per launch under steps_per_launch = 1, and under any trace, which asks for every step.
PATHS = {"wave-device-8": (DEVICE8, 1, False, False, 2 * L_STEPS // 8),                             # <1, 1, 0>
         "wave-host-trace": (dict(HOST, kernel=2), 3, True, False, 2 * L_STEPS),
         "k1": (dict(HOST, kernel=1), 2, True, False, 2 * L_STEPS),
         "server": (dict(persistent=1), 0, True, False, None),
         "wolf-device-8": (DEVICE8, 1, False, True, 2 * L_STEPS // 8),                              # <1, 1, 1>
         "wave-device-1-trace": (DEVICE1, 1, True, False, 2 * L_STEPS),                             # <1, 0, 0>
         "wolf-device-1-trace": (DEVICE1, 1, True, True, 2 * L_STEPS),                              # <1, 0, 1>
         "wave-device-8-perpair": (dict(DEVICE8, **PER_PAIR), 1, False, False, 2 * L_STEPS // 8),   # <0, 1, 0>
         "wolf-device-8-perpair": (dict(DEVICE8, **PER_PAIR), 1, False, True, 2 * L_STEPS // 8),    # <0, 1, 1>
         "wave-device-1-perpair-trace": (dict(DEVICE1, **PER_PAIR), 1, True, False, 2 * L_STEPS),   # <0, 0, 0>
         "wolf-device-1-perpair-trace": (dict(DEVICE1, **PER_PAIR), 1, True, True, 2 * L_STEPS),    # <0, 0, 1>
         "k0": (dict(HOST, kernel=0), 0, True, False, 2 * L_STEPS),
         "k4": (dict(HOST, kernel=4), 0, True, False, 2 * L_STEPS),
         "wolf-host-trace": (dict(HOST, kernel=2), 3, True, True, 2 * L_STEPS)}


def ladder_replay(r, T, wolf):
    return rp.replay_of("q216", False, L_REPLICA0 + r, ((L_STEPS, L_SEED, 0),), float(T), Q_DR, Q_DPHI, Q_RCUT, False,
                        wolf)


@pytest.mark.parametrize("wolf", [False, True])
def test_the_ladder_changes_a_decision_of_the_scalar_chain(wolf):
    """Host-side precondition of the next test: replayed at the scalar temperature handed to the
    call, a checked chain takes another accept decision than at its own temperature -- a run that
    ignored the array could not pass."""
    differ = [r for r in (4, 7)
              if [f for _, f in ladder_replay(r, L_TEMPS[r], wolf)["trace"]] !=
                 [f for _, f in ladder_replay(r, L_SCALAR, wolf)["trace"]]]
    assert differ == [4, 7], differ


@pytest.mark.parametrize("path", list(PATHS))
def test_laddered_chains_stepped_by_the_oracle(path, orc):
    """216 molecules, two sweeps, eight replicas at 250 ... 1000 K: every replica's final centres of
    mass, coordinates and S(k), the per-step trace where the path has one, and the totals against
    the replay at temps[r]; the launch count says which launch shape ran.  One chain for every
    path, so the replays are made once."""
    opts, n_parts, trace, wolf, launches = PATHS[path]
    a, _, _ = rp.system("q216", False)
    with open_batch(a, L_R, Q_RCUT, opts, wolf) as b:
        total = b.potential_wolf if wolf else b.potential_ewald
        t0 = total(as_array=True).copy()
        s_before = {r: b.get_replica(r)[2].copy() for r in range(L_R)}
        b.set_temperatures(L_TEMPS)
        assert np.array_equal(b.temperatures(), L_TEMPS)
        if trace:
            b.set_option("trace_steps", L_STEPS)
        e1, st = b.run(L_STEPS, L_SCALAR, Q_DR, Q_DPHI, seed=L_SEED, energies=t0["energy"].copy(), n_groups=2,
                       n_parts=n_parts, n_threads=2, replica0=L_REPLICA0)
        assert st["moves"] == L_R * L_STEPS
        assert st["device_decisions"] == (L_R * L_STEPS if opts.get("accept_on_device") else 0)
        assert st["server_steps"] == (L_STEPS if opts.get("persistent") == 1 else 0)
        assert launches is None or st["launches"] == launches, st      # (which launch shape ran)
        traces = b.get_trace(L_STEPS) if trace else None
        final = {r: b.get_replica(r) + (None,) for r in range(L_R)}
        t1 = total(as_array=True).copy()
    for r in range(L_R):
        o = ladder_replay(r, L_TEMPS[r], wolf)
        assert 0 < o["n_acc"] < L_STEPS
        if trace:
            rp._check_trace(o, *traces, r, path)
        if wolf:
            from test_gpu_wolf_paths import check_chain
            out = dict(t0=t0, e1=e1, t1=t1, traces=[], s_before=s_before, final=final)
            check_chain(orc, a, o, out, r, Q_RCUT, path)
        else:
            tot = {k: t1[k] for k in ("energy", "lj", "real", "recip")}
            rp._check_final(orc, a, o, final, r, t0["energy"], e1, tot, Q_RCUT, path)


# ---- 2. device and host decide alike under a ladder -------------------------------------------------
def _multi_record_run(a, opts, temps, style="ewald", n_steps=mr.N_STEPS, seed=mr.SEED):
    """One call of test_gpu_multi_record.py's shape on a fresh batch under `temps`: the running
    energies, the recomputed totals of the final state (the Wolf totals in Wolf style), the call's
    stats and every replica's state."""
    from metropolismontecarlo_amd import structs
    from metropolismontecarlo_amd.device import Batch
    with Batch(mr.R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"], 5.6 / a["box"],
               structs.factor, mr.RCUT, mr.RCUT) as b:
        b.set_option("device_moves", 1)
        for k, v in opts.items():
            b.set_option(k, v)
        total = b.potential_ewald
        if style == "wolf":
            b.recip_long()
            b.set_coulomb_style("wolf")
            total = b.potential_wolf
        b.set_temperatures(temps)
        e0 = total(as_array=True)["energy"].copy()
        e1, st = b.run(n_steps, mr.T, mr.DR, mr.DPHI, seed=seed, energies=e0, n_groups=2, n_parts=1, n_threads=2,
                       replica0=mr.REPLICA0)
        return e1, total(as_array=True).copy(), st, state_of(b)


def check_device_against_host(dev, host, n_steps, launches, at=None):
    """What the kernel's decisions left against what the host's left, each as _multi_record_run
    returns it: the six counts, every replica's centre of mass, coordinates and S(k) and the
    recomputed totals bit for bit, the running energies within test_gpu_multi_record.py's 1e-12 of
    each other and 1e-9 of the recompute; `launches` of the deciding kernel, a launch per step and
    group of the host's."""
    (e_d, t_d, st_d, fin_d), (e_h, t_h, st_h, fin_h) = dev, host
    assert st_d["launches"] == launches and st_d["device_decisions"] == mr.R * n_steps, (at, st_d)
    assert st_h["launches"] == 2 * n_steps and st_h["device_decisions"] == 0, (at, st_h)
    differ = [(r, what) for r in range(mr.R)
              for x, y, what in zip(fin_d[r], fin_h[r], ("com", "coords", "S(k)")) if not same_bits(x, y)]
    assert not differ, (at, differ)                      # (every replica that went another way, by index)
    assert [st_d[k] for k in mr.COUNTS] == [st_h[k] for k in mr.COUNTS], (at, st_d, st_h)
    assert 0 < st_d["trans_accept"] + st_d["rot_accept"] < mr.R * n_steps, at
    assert t_d.tobytes() == t_h.tobytes(), at
    print(at, "running energies, device against host:", np.max(np.abs(e_d - e_h) / np.abs(e_h)))
    assert np.max(np.abs(e_d - e_h) / np.abs(e_h)) < 1e-12, at
    print(at, "running energies against the recompute:", np.max(np.abs(e_d - t_d["energy"]) / np.abs(t_d["energy"])))
    assert np.max(np.abs(e_d - t_d["energy"]) / np.abs(t_d["energy"])) < 1e-9, at


def test_device_and_host_decide_alike_under_a_ladder():
    """NIST configuration 4, R = 24 in two groups, wave_wgs = 1, 20 steps in launches of 8 + 8 + 4
    (the shape of test_gpu_multi_record.py), twelve distinct temperatures: counts, centres of mass,
    coordinates and S(k) bit for bit between the kernel's decisions and the host's, running
    energies within that file's 1e-12 of each other and 1e-9 of the recompute.
    (test_gpu_tempering_paths.py: every kernel form and launch shape, a temperature per replica.)"""
    a = common.nist_arrays(4, "unwrapped")
    temps = np.tile(moves.geometric_ladder(260.0, 400.0, 12), 2)
    assert len(set(temps.tolist())) == 12
    check_device_against_host(_multi_record_run(a, mr.ON_DEVICE, temps), _multi_record_run(a, mr.ON_HOST, temps),
                              mr.N_STEPS, 2 * 3)


# ---- 3. off means off ---------------------------------------------------------------------------------
O_R, O_T, O_STEPS = 8, 300.0, 24
O_LADDER = moves.geometric_ladder(250.0, 1000.0, O_R)


def _two_calls(opts, n_parts, first, then, t1, t2):
    """A fresh batch through two calls (the Philox counter continues): set_temperatures(first) -- or
    nothing when `first` is the string "never" -- before call 1 at p->temperature t1, the same with
    `then` and t2 for call 2.  Returns what each call left: energies, counts, state."""
    a, _, _ = rp.system("q216", False)
    out = []
    with open_batch(a, O_R, Q_RCUT, opts) as b:
        e = b.potential_ewald(as_array=True)["energy"].copy()
        for k, (temps, t) in enumerate(((first, t1), (then, t2))):
            if not isinstance(temps, str):
                b.set_temperatures(temps)
            e, st = b.run(O_STEPS, t, Q_DR, Q_DPHI, seed=515 + k, energies=e, n_groups=2, n_parts=n_parts, n_threads=2,
                          replica0=40)
            out.append((e.copy(), [st[c] for c in mr.COUNTS], state_of(b)))
    return out


def _same_call(x, y):
    return same_bits(x[0], y[0]) and x[1] == y[1] and same_states(x[2], y[2])


@pytest.mark.parametrize("path", ["wave-device-8", "k1"])
def test_off_means_off(path):
    """An array of equal values, and set_temperatures(None) after a laddered call, each give the
    scalar chain bit for bit: the equal array against a fresh batch that never set one (two calls,
    so the Philox continuation is in it); None against a fresh batch that ran the same laddered
    call and then an array of equal values -- which the first half has shown to be the scalar
    chain.  p->temperature is 555 K wherever an array is set: it must be ignored."""
    opts, n_parts = PATHS[path][:2]
    equal = np.full(O_R, O_T)
    scalar = _two_calls(opts, n_parts, "never", "never", O_T, O_T)
    by_array = _two_calls(opts, n_parts, equal, "same", 555.0, 555.0)
    assert _same_call(scalar[0], by_array[0]) and _same_call(scalar[1], by_array[1])
    off_again = _two_calls(opts, n_parts, O_LADDER, None, 555.0, O_T)
    equal_again = _two_calls(opts, n_parts, O_LADDER, equal, 555.0, 555.0)
    assert _same_call(off_again[0], equal_again[0]) and _same_call(off_again[1], equal_again[1])
    assert not _same_call(scalar[0], off_again[0])          # (the laddered call was another chain)


# ---- 4. exchange through the batch ----------------------------------------------------------------------
X_R, X_RUNGS, X_ROUNDS, X_STEPS, X_SEED, X_REPLICA0, X_ROUND0 = 12, 4, 6, 40, 6021, 24, 3
X_LADDER = moves.geometric_ladder(250.0, 1000.0, X_RUNGS)


class OracleChain:
    """test_gpu_replay_paths.replay in steps, for a chain whose temperature changes between calls:
    advance(n_steps, T) is one call of the batch (the Philox counter continues, the sweep restarts).
    e_acc is the running sum of the accepted dU.  `wolf`: the chain of replay(wolf=True) --
    dU = d_lj + d_real, the S arrays left alone."""

    def __init__(self, orc, a, replica, seed, dr, dphi, rcut, wolf=False):
        self.orc, self.box, self.n_mol = orc, a["box"], a["com"].shape[0]
        self.key, self.par = (seed, replica), (dr, dphi, rcut)
        self.s = common.oracle_system(a)
        self.ew = orc.Ewald(5.6 / self.box, 5, 27, self.box)
        orc.recip_long(self.ew, self.s.coords, self.s.charge, self.box)
        self.e_acc, self.off, self.wolf = 0.0, 0, wolf

    def advance(self, n_steps, T):
        s, ew, (dr, dphi, rcut) = self.s, self.ew, self.par
        for step in range(n_steps):
            i = step % self.n_mol
            _, c_new, a_new, _, u = rp.propose(0, *self.key, self.off + step, s.com[i].copy(),
                                               s.coords[3 * i:3 * i + 3].copy(), None, None, self.box, dr, dphi)
            d, ov = self.orc.trial_move(i + 1, s, ew, rcut, rcut, c_new, a_new)
            delta = d[0] + d[1] if self.wolf else d[0] + d[1] + d[2]   # main.jl:593
            x = delta / T
            if (x < 0.0 or math.exp(-x) > u) and not ov:               # main.jl:598
                self.e_acc += delta
                s.com[i] = c_new
                s.coords[3 * i:3 * i + 3] = a_new
                if not self.wolf:
                    ew.sumQExpOld = ew.sumQExpNew.copy()
            elif not self.wolf:
                ew.sumQExpNew = ew.sumQExpOld.copy()
        self.off += n_steps
        return self

    def result(self):
        return dict(com=self.s.com, coords=self.s.coords, S=self.ew.sumQExpOld, quat=None, e_acc=self.e_acc)


def replay_rounds(orc, a, replica, temps_of_round):
    c = OracleChain(orc, a, replica, X_SEED, Q_DR, Q_DPHI, Q_RCUT)
    for T in temps_of_round:
        c.advance(X_STEPS, float(T))
    return c.result()


@functools.lru_cache(maxsize=None)
def oracle_ladder_run(wolf=False, ladder=tuple(X_LADDER)):
    """The whole run of test 4 on the host: every chain stepped by the oracle, every exchange decided
    by the restatement on the oracle's energies (all replicas start from one configuration, so the
    start's energy drops out of every D).  Returns the temperature history and the counters."""
    from oracle import oracle as orc
    a, _, _ = rp.system("q216", False)
    chains = [OracleChain(orc, a, X_REPLICA0 + r, X_SEED, Q_DR, Q_DPHI, Q_RCUT, wolf) for r in range(X_R)]
    temps, rung = np.tile(ladder, X_R // X_RUNGS).tolist(), moves.initial_rungs(X_R, X_RUNGS).tolist()
    attempt, accept, t_hist = [0] * (X_RUNGS - 1), [0] * (X_RUNGS - 1), [list(temps)]
    for i in range(X_ROUNDS):
        e = [chains[r].advance(X_STEPS, temps[r]).e_acc for r in range(X_R)]
        rnd = X_ROUND0 + i
        assert tempering_ref.exchange_round(X_R // X_RUNGS, X_RUNGS, rnd & 1, X_SEED, X_REPLICA0, rnd, 0.0, e, None,
                                            temps, rung, attempt, accept)
        t_hist.append(list(temps))
    return dict(temps=t_hist, attempt=attempt, accept=accept)


def test_the_ladder_spacing_accepts_and_rejects_swaps():
    """Host-side precondition of the next test, from the oracle: in its 6 rounds at least one swap
    is accepted and at least one rejected."""
    o = oracle_ladder_run()
    assert sum(o["accept"]) >= 1 and sum(o["attempt"]) - sum(o["accept"]) >= 1, o


X_KW = dict(n_groups=2, n_threads=2, replica0=X_REPLICA0)


def exchange_whole(opts, n_parts=1, wolf=False):
    """run_exchange of X_ROUNDS x X_STEPS on a fresh batch of X_R // X_RUNGS ladders: what it left
    (energies, rung, temperatures(), state, counters), the stats, the totals before and after."""
    a, _, _ = rp.system("q216", False)
    with open_batch(a, X_R, Q_RCUT, opts, wolf) as b:
        total = b.potential_wolf if wolf else b.potential_ewald
        t0 = total(as_array=True).copy()
        b.set_temperatures(np.tile(X_LADDER, X_R // X_RUNGS))
        rung = moves.initial_rungs(X_R, X_RUNGS)
        e1, st, attempt, accept = b.run_exchange(X_ROUNDS, X_STEPS, Q_DR, Q_DPHI, X_SEED, t0["energy"].copy(), rung,
                                                 X_RUNGS, round0=X_ROUND0, temperature=555.0, n_parts=n_parts, **X_KW)
        assert st["moves"] == X_R * X_ROUNDS * X_STEPS, st
        whole = dict(e=e1, rung=rung, temps=b.temperatures(), state=state_of(b), attempt=attempt, accept=accept)
        return whole, st, t0, total(as_array=True).copy()


def exchange_by_hand(decide, opts, n_parts=1, wolf=False):
    """The same run composed from run, set_temperatures and decide(round, energies, temps, rung,
    attempt, accept) -> (temps, rung).  Returns what it left and the temperatures after each round."""
    a, _, _ = rp.system("q216", False)
    with open_batch(a, X_R, Q_RCUT, opts, wolf) as b:
        e = (b.potential_wolf if wolf else b.potential_ewald)(as_array=True)["energy"].copy()
        temps, rung = np.tile(X_LADDER, X_R // X_RUNGS), moves.initial_rungs(X_R, X_RUNGS)
        att, acc = np.zeros(X_RUNGS - 1, np.int64), np.zeros(X_RUNGS - 1, np.int64)
        t_hist = [temps.copy()]
        for i in range(X_ROUNDS):
            b.set_temperatures(temps)
            e, _ = b.run(X_STEPS, 555.0, Q_DR, Q_DPHI, seed=X_SEED, energies=e, n_parts=n_parts, **X_KW)
            temps, rung = decide(X_ROUND0 + i, e, temps, rung, att, acc)
            t_hist.append(temps.copy())
        b.set_temperatures(temps)
        return dict(e=e, rung=rung, temps=b.temperatures(), state=state_of(b), attempt=att, accept=acc), t_hist


def decide_pure(rnd, e, temps, rung, att, acc):
    exchange_round(X_RUNGS, e, temps, rung, X_SEED, rnd, replica0=X_REPLICA0, attempt=att, accept=acc)
    return temps, rung


def decide_restated(rnd, e, temps, rung, att, acc):
    t, g, at, ac = temps.tolist(), rung.tolist(), att.tolist(), acc.tolist()
    assert tempering_ref.exchange_round(X_R // X_RUNGS, X_RUNGS, rnd & 1, X_SEED, X_REPLICA0, rnd, 0.0, e.tolist(),
                                        None, t, g, at, ac)
    att[:], acc[:] = at, ac
    return np.array(t), np.array(g, dtype=np.int32)


def check_exchange_composition(whole, hand, at):
    """Bit for bit: energies, rung, temperatures(), the counters and every replica's state; the
    temperatures are the ladder's at the rungs held; swaps were accepted and rejected."""
    attempt, accept = whole["attempt"], whole["accept"]
    assert np.array_equal(whole["temps"], X_LADDER[whole["rung"]]), at
    assert attempt.tolist() == [9, 9, 9] and accept.sum() >= 1 and (attempt - accept).sum() >= 1, (at, attempt, accept)
    for key in ("e", "rung", "temps", "attempt", "accept"):
        assert same_bits(whole[key], hand[key]), (at, key, whole[key], hand[key])
    assert same_states(whole["state"], hand["state"]), at


def test_run_exchange_is_run_and_exchange_composed_by_hand(orc):
    """R = 12 as 3 ladders of 4 rungs: run_exchange of 6 rounds x 40 steps equals, bit for bit in
    final state, energies, rung and temperatures(), the same thing composed from run and the pure
    exchange_round, and from run and the restatement; swaps are accepted and rejected; and a
    replica whose temperature an accepted swap changed follows the oracle's replay at its new
    temperatures in the rounds after."""
    a, _, _ = rp.system("q216", False)
    whole, st, t0, tot = exchange_whole(DEVICE8)
    e0 = t0["energy"]
    assert st["device_decisions"] == st["moves"]
    for decide in (decide_pure, decide_restated):
        hand, t_hist = exchange_by_hand(decide, DEVICE8)
        check_exchange_composition(whole, hand, decide.__name__)
    # a replica whose temperature changed before the last round, against the oracle at its history
    t_hist = np.array(t_hist)                                            # [round + 1, R]
    moved = [r for r in range(X_R) if (t_hist[1:X_ROUNDS, r] != t_hist[0, r]).any()]
    assert moved
    r = moved[0]
    o = replay_rounds(orc, a, X_REPLICA0 + r, t_hist[:X_ROUNDS, r])
    final = {r: whole["state"][r] + (None,)}
    rp._check_final(orc, a, o, final, r, e0, whole["e"], {k: tot[k] for k in ("energy", "lj", "real", "recip")},
                    Q_RCUT, "after a swap")
    # ... and held at its first temperature throughout it would have been another chain
    stay = replay_rounds(orc, a, X_REPLICA0 + r, [t_hist[0, r]] * X_ROUNDS)
    assert not np.array_equal(stay["com"], o["com"])


# ---- 5. per-replica boxes ---------------------------------------------------------------------------------
def test_per_replica_boxes_use_each_replicas_beta(orc):
    """R = 4 in two boxes under 280 K and 350 K: one run_npt_replicas(n_sweeps = 1) against the same
    sweep composed by hand -- run, volume_trial_replicas, each replica's criterion recomputed on the
    host at its own beta (volumeChange.jl:129-132), volume_settle -- bit for bit.  The pressure is
    large enough to decide the sign of the exponent, so that against the scalar temperature handed
    to the call (1e9 K: beta = 0) the decision of every expanding replica differs: asserted.  Then
    one exchange with that pressure against the restatement fed get_boxes() ** 3."""
    import ctypes
    import ctypes.util
    from test_gpu_moves import philox_pair
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.cbrt.restype, libm.cbrt.argtypes = ctypes.c_double, [ctypes.c_double]
    from test_gpu_npt_replicas import ALPHA, DPHI, DR, nist4_boxes, per_box_batch
    states = nist4_boxes((0.99, 0.99, 1.02, 1.02))
    R, n_mol, seed, replica0, per_sweep, pressure, t_scalar = 4, 750, 2719, 8, 30, 100.0, 1.0e9
    temps = np.array([280.0, 350.0, 280.0, 350.0])
    vmax = 0.02 * states[0]["box"] ** 3
    kw = dict(moves_per_sweep=per_sweep, alpha=ALPHA, replica0=replica0)
    with per_box_batch(states) as b:
        b.set_temperatures(temps)
        e0 = b.potential_ewald(as_array=True)["energy"].copy()
        e1, st, ns = b.run_npt_replicas(1, t_scalar, pressure, vmax, DR, DPHI, seed, e0, **kw)
        got = dict(e=e1, boxes=b.get_boxes(), state=state_of(b), acc=[x["vol_accept"] for x in ns])
    with per_box_batch(states) as b:
        b.set_temperatures(temps)
        e, _ = b.run(per_sweep, t_scalar, DR, DPHI, seed=seed, energies=e0, n_groups=1, n_threads=1, replica0=replica0)
        boxes = b.get_boxes()
        draws = [philox_pair(seed, replica0 + r, per_sweep, 0x40000000) for r in range(R)]       # MMC_SLOT_VOLUME
        vol_old = boxes * boxes * boxes
        vol_new = np.array([vol_old[r] + (draws[r][0] - 0.5) * vmax for r in range(R)])
        new_boxes = np.array([libm.cbrt(v) for v in vol_new])                                   # (the C library's cbrt)
        assert (new_boxes / 2 >= 10.0).all()
        tot = b.volume_trial_replicas(new_boxes)

        def decide(r, beta):
            arg = -beta * (pressure * (vol_new[r] - vol_old[r]) - n_mol * math.log(vol_new[r] / vol_old[r]) / beta
                           + (tot["energy"][r] - e[r])) if beta else n_mol * math.log(vol_new[r] / vol_old[r])
            return draws[r][1] < math.exp(min(arg, 700.0))

        own = [decide(r, 1.0 / temps[r]) for r in range(R)]
        at_scalar = [decide(r, 0.0) for r in range(R)]
        assert any(x != y for x, y in zip(own, at_scalar)), (own, at_scalar, vol_new - vol_old)
        b.volume_settle(np.array(own, dtype=np.int32))
        e = np.where(own, tot["energy"], e)
        assert got["acc"] == [int(x) for x in own]
        assert same_bits(got["boxes"], b.get_boxes()) and same_bits(got["e"], e)
        assert same_states(got["state"], state_of(b))
        # one exchange with the pressure: two ladders of two rungs
        rung = moves.initial_rungs(R, 2)
        att, acc = b.exchange(2, e, rung, seed, 0, pressure=pressure, replica0=replica0)
        t, g, at, ac = temps.tolist(), [0, 1, 0, 1], [0], [0]
        bx = b.get_boxes()
        assert tempering_ref.exchange_round(2, 2, 0, seed, replica0, 0, pressure, e.tolist(), (bx * bx * bx).tolist(),
                                            t, g, at, ac)
        assert b.temperatures().tolist() == t and rung.tolist() == g and att.tolist() == at and acc.tolist() == ac


# ---- 6. state errors ----------------------------------------------------------------------------------------
def test_state_errors():
    a, _, _ = rp.system("q216", False)
    with open_batch(a, 6, Q_RCUT, dict(persistent=0)) as b:
        e = b.potential_ewald(as_array=True)["energy"].copy()
        rung = moves.initial_rungs(6, 3)
        with pytest.raises(MMCError, match="MMC_ERR_STATE"):
            b.exchange(3, e, rung, 1, 0)                               # before set_temperatures
        with pytest.raises(MMCError, match="MMC_ERR_STATE"):
            b.run_exchange(1, 4, Q_DR, Q_DPHI, 1, e, rung, 3)
        assert np.array_equal(b.temperatures(), np.zeros(6))
        with pytest.raises(MMCError, match="MMC_ERR_ARG"):
            b.set_temperatures([300.0, 300.0, -1.0, 300.0, 300.0, 300.0])
        with pytest.raises(MMCError, match="MMC_ERR_ARG"):
            b.set_temperatures([300.0, np.inf, 300.0, 300.0, 300.0, 300.0])
        assert np.array_equal(b.temperatures(), np.zeros(6))             # no state changed
        b.set_temperatures(np.tile([250.0, 300.0, 360.0], 2))
        with pytest.raises(MMCError, match="MMC_ERR_ARG"):
            b.exchange(4, e, moves.initial_rungs(8, 4)[:6].copy(), 1, 0)   # 6 replicas, 4 rungs
        with pytest.raises(MMCError, match="MMC_ERR_ARG"):
            b.run_exchange(1, 4, Q_DR, Q_DPHI, 1, e, rung, 4)
        with pytest.raises(MMCError, match="MMC_ERR_ARG"):
            b.run_exchange(1, 4, Q_DR, Q_DPHI, 1, e, np.zeros(6, np.int32), 3)   # not a permutation: before any move
        assert same_bits(b.potential_ewald(as_array=True)["energy"], e)
        assert rung.tolist() == [0, 1, 2, 0, 1, 2]
        assert np.array_equal(b.temperatures(), np.tile([250.0, 300.0, 360.0], 2))
    with open_batch(a, 1, Q_RCUT, dict()) as b1:
        e = float(b1.potential_ewald(as_array=True)["energy"][0])
        b1.set_temperatures([300.0])
        with pytest.raises(MMCError, match="MMC_ERR_UNSUPPORTED"):
            b1.run_npt(1, 300.0, 0.0, 100.0, Q_DR, Q_DPHI, 1, e)
        b1.set_temperatures(None)
        assert b1.temperatures().tolist() == [0.0]
