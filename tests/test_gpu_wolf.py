"""Wolf-style chains of the replica batch (mmc_batch_set_coulomb_style; the reference's global
`Wolf = true`, Ewald/main.jl:75): every step against the oracle on every move kernel, S(k) left
alone, the Wolf total (energy.jl:864-943), run_chains, eval / settle, the untouched default and
the fences.

replay_wolf() is test_gpu_replay_paths.replay(wolf=True): dU = d_lj + d_real (main.jl:580-593
with Wolf: deltaRecip = 0) and no commit or rollback of the oracle's S arrays.
Tolerances as there: TOL * (|dU| + 1e4) per step, flags exact, 2e-13 A on coordinates,
TOL * 1e5 on a call's energy change.

The virial of a Wolf chain: the reference's Loop() adds (partial_new_v - partial_old_v) per
accepted move, and partial_*_v carries EwaldShort's virial e/3 (main.jl:566-568, :600-601), while
its Wolf potential() adds NO virial for the real part (energy.jl:919-920).  A chain's virial
change therefore equals the change of potential_wolf's `virial + real / 3`, not of `virial`
alone; test_run_chains_against_the_recompute compares with that, from potential_wolf's own two
fields, at the tolerance of 1e-9 relative to the magnitudes the difference is formed from."""
import functools

import numpy as np
import pytest

import common
from common import rel
from test_gpu_replay_paths import make_batch, replay, system

pytestmark = pytest.mark.gpu

TOL = 1e-9
Q_RCUT, Q_T, Q_DR, Q_DPHI = 7.0, 298.15, 0.3, 0.3
Q_STEPS = 2 * 216 + 5                      # two sweeps and the start of a third
R8, SEED, REPLICA0, CHECK = 8, 31337, 11, (0, 3, 4, 7)
C4_RCUT, C4_STEPS = 10.0, 40


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@functools.lru_cache(maxsize=None)
def arrays(name):
    if name == "cfg4":
        return common.nist_arrays(4, "unwrapped")
    return system(name, False)[0]


def oracle_ewald(orc, a):
    return orc.Ewald(5.6 / a["box"], 5, 27, a["box"])


def replay_wolf(orc, a, replica, calls, T, dr, dphi, rcut):
    """One Wolf chain on the host (rigid device-made moves) through the calls [(n_steps, seed), ...]:
    test_gpu_replay_paths.replay(wolf=True), see the module docstring."""
    return replay(orc, a, replica, [(n, seed, 0) for n, seed in calls], T, dr, dphi, rcut, wolf=True)


@functools.lru_cache(maxsize=None)
def replay_of(name, replica, calls, T, dr, dphi, rcut):
    from oracle import oracle as orc
    return replay_wolf(orc, arrays(name), replica, calls, T, dr, dphi, rcut)


def check_totals(orc, a, com, coords, t, rcut, at):
    """One replica's potential_wolf record `t` against orc.potential_wolf of (com, coords)."""
    s = common.oracle_system(dict(a, com=com, coords=coords))
    to = orc.potential_wolf(s, oracle_ewald(orc, a), rcut, rcut)
    for key in ("energy", "lj", "real", "self"):
        assert rel(t[key], to[key]) < TOL, (at, key, t[key], to[key])
    assert t["recip"] == 0.0 and t["n_overlap"] == to["n_overlap"], (at, t["recip"])


def run_wolf(a, R, rcut, opts, n_steps, seed, check, trace, n_parts, replica0, T=Q_T, dr=Q_DR, dphi=Q_DPHI):
    """A Wolf run of one batch.  Returns energies before / after by potential_wolf and by the run,
    the trace, S(k) before and after and the final state of the replicas in `check`, the stats."""
    with make_batch(a, R, rcut) as b:
        b.set_option("device_moves", 1)
        for k, v in opts.items():
            b.set_option(k, v)
        b.recip_long()                          # S(k) of the start: what a Wolf run must leave alone
        b.set_coulomb_style("wolf")
        assert b.coulomb_style == "wolf"
        t0 = b.potential_wolf(as_array=True).copy()
        s_before = {r: b.get_replica(r)[2].copy() for r in check}
        if trace:
            b.set_option("trace_steps", n_steps)
        e1, st = b.run(n_steps, T, dr, dphi, seed=seed, energies=t0["energy"], n_groups=2, n_parts=n_parts,
                       n_threads=2, replica0=replica0)
        tr = b.get_trace(n_steps) if trace else None
        final = {r: b.get_replica(r) for r in check}
        t1 = b.potential_wolf(as_array=True).copy()
        assert b.coulomb_style == "wolf"
    return t0, e1, t1, tr, s_before, final, st


def check_run(orc, name, a, rcut, n_steps, seed, replica0, check, t0, e1, t1, tr, s_before, final, at):
    n_rej = 0
    for r in check:
        o = replay_of(name, replica0 + r, ((n_steps, seed),), Q_T, Q_DR, Q_DPHI, rcut)
        if tr is not None:                                    # every step: dU and the flag byte
            for step, (delta, flags) in enumerate(o["trace"]):
                assert abs(tr[0][r, step] - delta) < TOL * (abs(delta) + 1e4), (at, r, step, tr[0][r, step], delta)
                assert tr[1][r, step] == flags, (at, r, step, tr[1][r, step], flags)
        com, coords, S = final[r]
        assert np.abs(com - o["com"]).max() < 2e-13 and np.abs(coords - o["coords"]).max() < 2e-13, (at, r)
        assert np.array_equal(S.view(np.uint64), s_before[r].view(np.uint64)), (at, r, "S(k) touched")
        assert abs((e1[r] - t0["energy"][r]) - o["e_acc"]) < TOL * 1e5, (at, r)
        # the reference's recompute check (Poly/main.jl:232-235) on the batch's own Wolf total
        assert abs((e1[r] - t0["energy"][r]) - (t1["energy"][r] - t0["energy"][r])) < TOL * 1e5, (at, r)
        check_totals(orc, a, a["com"], a["coords"], t0[r], rcut, (at, r, "start"))
        check_totals(orc, a, com, coords, t1[r], rcut, (at, r, "final"))
        n_rej += n_steps - o["n_acc"]
    return n_rej


# ---- 1-3: every step on every kernel, S(k) untouched, the totals ----------------------------------
@pytest.mark.parametrize("opts,parts,decides,per_launch", [
    pytest.param(dict(kernel=2, persistent=0, accept_on_device=0), 3, 0, 1, id="k2-host-3parts"),
    pytest.param(dict(kernel=2, persistent=0, accept_on_device=1, steps_per_launch=1), 1, 1, 1, id="k2-device-1"),
    pytest.param(dict(kernel=2, persistent=0, accept_on_device=1, steps_per_launch=8), 1, 1, 8, id="k2-device-8"),
    pytest.param(dict(kernel=1, accept_on_device=0), 2, 0, 1, id="k1-2parts"),
    pytest.param(dict(kernel=0, persistent=0, accept_on_device=0), 0, 0, 1, id="k0")])
def test_wolf_chain_stepped_by_the_oracle(opts, parts, decides, per_launch, orc):
    """216 molecules (r_cut 7 A), two sweeps + 5 steps, eight replicas in two groups, replicas at both
    ends of both groups checked.  Where a launch takes one step: every step's dU and flags.  Eight
    steps per launch (no trace on that path): accept and overlap counts of all eight replicas, final
    coordinates, the energy change.  Always: S(k) bitwise untouched, potential_wolf of the start and
    of the final state against the oracle, the running total against the recompute.  The k1 case
    leaves `persistent` at -1: a Wolf batch simply uses launches."""
    a = arrays("q216")
    trace = per_launch == 1
    check = CHECK if trace else tuple(range(R8))
    out = run_wolf(a, R8, Q_RCUT, opts, Q_STEPS, SEED, check, trace, parts, REPLICA0)
    st = out[-1]
    assert st["moves"] == R8 * Q_STEPS and st["server_steps"] == 0, st
    assert st["device_decisions"] == (R8 * Q_STEPS if decides else 0), st
    n_rej = check_run(orc, "q216", a, Q_RCUT, Q_STEPS, SEED, REPLICA0, check, *out[:-1], at=opts)
    assert n_rej > 20
    if not trace:
        assert st["launches"] == 2 * -(-Q_STEPS // per_launch), st
        os_ = [replay_of("q216", REPLICA0 + r, ((Q_STEPS, SEED),), Q_T, Q_DR, Q_DPHI, Q_RCUT) for r in range(R8)]
        assert st["trans_accept"] + st["rot_accept"] == sum(o["n_acc"] for o in os_), st
        assert st["overlaps"] == sum(o["n_ovl"] for o in os_), st
        assert st["rot_attempt"] == sum(o["n_rot"] for o in os_), st


def test_wolf_chain_on_nist_configuration_4(orc):
    """750 molecules, r_cut 10 A, 40 steps on kernel 2 with the kernel's own decision."""
    a = arrays("cfg4")
    opts = dict(kernel=2, persistent=0, accept_on_device=1, steps_per_launch=1)
    out = run_wolf(a, R8, C4_RCUT, opts, C4_STEPS, SEED, CHECK, True, 1, REPLICA0)
    assert out[-1]["device_decisions"] == R8 * C4_STEPS, out[-1]
    check_run(orc, "cfg4", a, C4_RCUT, C4_STEPS, SEED, REPLICA0, CHECK, *out[:-1], at="cfg4")


def test_wolf_moves_leave_sk_alone_after_ewald_moves(orc):
    """After an Ewald run the two S(k) buffers of a replica differ (the last rejected trial) and
    sumQExpOld may be either: a Wolf run must leave get_replica's sum_old bit for bit what it was,
    on the host-decided, the device-decided and the several-steps-per-launch paths."""
    a = arrays("q216")
    for opts, parts in ((dict(kernel=2, persistent=0, accept_on_device=0), 3),
                        (dict(kernel=2, persistent=0, accept_on_device=1, steps_per_launch=1), 1),
                        (dict(kernel=2, persistent=0, accept_on_device=1, steps_per_launch=8), 1),
                        (dict(kernel=1, persistent=0, accept_on_device=0), 2)):
        with make_batch(a, R8, Q_RCUT) as b:
            b.set_option("device_moves", 1)
            for k, v in opts.items():
                b.set_option(k, v)
            e = b.potential_ewald(as_array=True)["energy"].copy()
            e, _ = b.run(61, Q_T, Q_DR, Q_DPHI, seed=5, energies=e, n_parts=parts, n_threads=2)
            before = [b.get_replica(r)[2].copy() for r in range(R8)]
            b.set_coulomb_style("wolf")
            _, st = b.run(75, Q_T, Q_DR, Q_DPHI, seed=6, energies=b.potential_wolf(as_array=True)["energy"],
                          n_parts=parts, n_threads=2)
            assert 0 < st["trans_accept"] + st["rot_accept"] < st["moves"]
            for r in range(R8):
                assert np.array_equal(b.get_replica(r)[2].view(np.uint64), before[r].view(np.uint64)), (opts, r)


# ---- 3: the Wolf total ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,rcut", [("q216", Q_RCUT), ("cfg4", C4_RCUT)])
@pytest.mark.parametrize("R", [1, 3])
def test_potential_wolf_against_the_oracle(name, rcut, R, orc):
    """potential_wolf of distinct configurations per replica, in either style, as dicts and as a
    record array; it does not touch S(k)."""
    a = arrays(name)
    cases = [a, dict(a, com=a["com"] + 0.37, coords=a["coords"] + 0.37),
             dict(a, com=a["com"][::-1].copy(), coords=a["coords"].reshape(-1, 3, 3)[::-1].reshape(-1, 3).copy())][:R]
    with make_batch(a, R, rcut) as b:
        for r, c in enumerate(cases):
            b.set_replica(r, c["com"], c["coords"])
        b.recip_long()
        s0 = [b.get_replica(r)[2].copy() for r in range(R)]
        for style in ("ewald", "wolf"):
            b.set_coulomb_style(style)
            tot, arr = b.potential_wolf(), b.potential_wolf(as_array=True)
            for r, c in enumerate(cases):
                check_totals(orc, a, c["com"], c["coords"], tot[r], rcut, (name, R, style, r))
                assert tot[r]["energy"] == arr["energy"][r] and tot[r]["virial"] == arr["virial"][r]
                s = common.oracle_system(c)
                to = orc.potential_wolf(s, oracle_ewald(orc, a), rcut, rcut)
                assert rel(tot[r]["virial"], to["virial"]) < TOL, (name, r)
        for r in range(R):
            assert np.array_equal(b.get_replica(r)[2].view(np.uint64), s0[r].view(np.uint64))


# ---- 4: run_chains --------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,parts", [(2, 1), (1, 2)])
def test_run_chains_against_the_recompute(kernel, parts):
    """adjust = 1 over two sweeps in Wolf style: mmc_chain.energy against potential_wolf of the final
    state, and the chain's virial change against the change of potential_wolf's virial + real / 3
    (module docstring), to 1e-9 relative of the magnitudes the differences are formed from."""
    a = arrays("q216")
    with make_batch(a, R8, Q_RCUT) as b:
        b.set_option("device_moves", 1)
        b.set_option("kernel", kernel)
        b.set_coulomb_style("wolf")
        t0 = b.potential_wolf(as_array=True).copy()
        v0 = t0["virial"] + t0["real"] / 3
        chains = b.new_chains(t0["energy"], v0, dr_max=Q_DR, dphi_max=Q_DPHI)
        st = b.run_chains(chains, 2 * 216, Q_T, seed=77, adjust=True, n_parts=parts, n_threads=2)
        assert st["moves"] == R8 * 2 * 216 and st["server_steps"] == 0
        t1 = b.potential_wolf(as_array=True)
        v1 = t1["virial"] + t1["real"] / 3
        for r in range(R8):
            assert abs(chains["energy"][r] - t1["energy"][r]) < TOL * 1e5, (r, chains["energy"][r], t1["energy"][r])
            dv_chain, dv_tot = chains["virial"][r] - v0[r], v1[r] - v0[r]
            scale = abs(chains["virial"][r]) + abs(v0[r]) + abs(v1[r])
            assert abs(dv_chain - dv_tot) < TOL * scale, (r, dv_chain, dv_tot, scale)
            assert chains["steps_taken"][r] == 2 * 216 and 0 < chains["trans_naccept"][r] < chains["trans_attempt"][r]
        assert (chains["dr_max"] != Q_DR).any()          # the step sizes were adapted


def test_run_chains_virial_against_the_oracle(orc):
    """Fixed step sizes (adjust = 0), so the chains are replay_wolf's: mmc_chain.energy and .virial
    changes of the replicas at both ends of both groups against the oracle's own sums of the
    accepted moves' dU and d_vir (orc.trial_move's d_vir without its d_recip / 3)."""
    a = arrays("q216")
    with make_batch(a, R8, Q_RCUT) as b:
        b.set_option("device_moves", 1)
        b.set_option("kernel", 2)
        b.set_coulomb_style("wolf")
        t0 = b.potential_wolf(as_array=True).copy()
        v0 = t0["virial"] + t0["real"] / 3
        chains = b.new_chains(t0["energy"], v0, dr_max=Q_DR, dphi_max=Q_DPHI)
        b.run_chains(chains, Q_STEPS, Q_T, seed=SEED, adjust=False, n_parts=1, n_threads=2, replica0=REPLICA0)
        for r in CHECK:
            o = replay_of("q216", REPLICA0 + r, ((Q_STEPS, SEED),), Q_T, Q_DR, Q_DPHI, Q_RCUT)
            assert abs((chains["energy"][r] - t0["energy"][r]) - o["e_acc"]) < TOL * 1e5, r
            dv = chains["virial"][r] - v0[r]
            assert abs(dv - o["v_acc"]) < TOL * (abs(chains["virial"][r]) + abs(v0[r]) + abs(o["v_acc"])), (r, dv, o["v_acc"])
            assert chains["trans_naccept"][r] + chains["rot_naccept"][r] == o["n_acc"], r


# ---- 5: eval / settle -----------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,parts", [(2, 1), (2, 3), (1, 2), (0, 3)])
def test_eval_and_settle_in_wolf_style(kernel, parts, orc):
    """Scripted moves through mmc_batch_eval in Wolf style: d_recip == 0.0 exactly; d_lj, d_real,
    d_vir (the oracle's without its d_recip / 3) and overlap against orc.trial_move.  Move 3 puts
    the oxygen of molecule 4 at 0.4 A from a hydrogen of molecule 10: an overlap."""
    a = arrays("q216")
    R, rng = 3, np.random.default_rng(12)
    rules = [lambda n: True, lambda n: False, lambda n: n % 2 == 0]
    s = [common.oracle_system(a) for _ in range(R)]
    ew = [oracle_ewald(orc, a) for _ in range(R)]
    for r in range(R):
        orc.recip_long(ew[r], s[r].coords, s[r].charge, a["box"])
    n_ovl = 0
    with make_batch(a, R, Q_RCUT) as b:
        b.set_option("kernel", kernel)
        b.set_parts(parts)
        b.recip_long()
        b.set_coulomb_style("wolf")
        s_before = [b.get_replica(r)[2].copy() for r in range(R)]
        acc_prev = np.zeros(R, dtype=bool)
        for n in range(8):
            mol = 1 + (n * 5) % 216
            i = mol - 1
            com_new, at_new = np.empty((R, 3)), np.empty((R, 3, 3))
            for r in range(R):
                shift = (rng.random(3) - 0.5) * 0.6
                if n == 3:   # the oxygen (atom 0) onto a hydrogen of molecule 10, 0.4 A off
                    shift = s[r].coords[3 * 9 + 1] + np.array([0.4, 0.0, 0.0]) - s[r].coords[3 * i]
                com_new[r] = s[r].com[i] + shift
                at_new[r] = s[r].coords[3 * i:3 * i + 3] + shift
            d, ov = b.eval(mol, com_new, at_new, acc_prev)
            for r in range(R):
                do, ovo = orc.trial_move(mol, s[r], ew[r], Q_RCUT, Q_RCUT, com_new[r], at_new[r])
                want = np.array([do[0], do[1], do[3] - do[2] / 3])
                assert ov[r] == ovo, (n, r)
                assert d[r][2] == 0.0, (n, r, d[r][2])
                assert np.abs(d[r][[0, 1, 3]] - want).max() < TOL * (np.abs(want).max() + 1e4), (n, r, d[r], want)
                n_ovl += ovo
                acc = rules[r](n) and not ovo
                if acc:
                    s[r].com[i] = com_new[r]
                    s[r].coords[3 * i:3 * i + 3] = at_new[r]
                acc_prev[r] = acc
        b.settle(acc_prev)
        for r in range(R):
            com, coords, S = b.get_replica(r)
            assert np.array_equal(com, s[r].com) and np.array_equal(coords, s[r].coords), r
            assert np.array_equal(S.view(np.uint64), s_before[r].view(np.uint64)), r
    assert n_ovl >= R


# ---- 6: the default is untouched ------------------------------------------------------------------
@pytest.mark.parametrize("opts,parts", [
    (dict(kernel=2, persistent=0, accept_on_device=0), 3),
    (dict(kernel=2, persistent=0, accept_on_device=1, steps_per_launch=1), 1),
    (dict(kernel=1, persistent=0, accept_on_device=0), 2), (dict(kernel=0, persistent=0), 0)])
def test_default_style_is_untouched(opts, parts):
    """Batch A never touches the style; B sets Wolf, sets Ewald, calls recip_long, then runs: the
    same traces, final coordinates and S(k), bit for bit.  Between B's switch back and its
    recip_long, run returns MMC_ERR_STATE naming mmc_batch_recip_long."""
    from metropolismontecarlo_amd._lib import MMCError
    a = arrays("q216")
    n_steps, got = 150, []
    for switch in (False, True):
        with make_batch(a, R8, Q_RCUT) as b:
            b.set_option("device_moves", 1)
            for k, v in opts.items():
                b.set_option(k, v)
            e0 = b.potential_ewald(as_array=True)["energy"].copy()
            assert b.coulomb_style == "ewald"
            if switch:
                b.set_coulomb_style("wolf")
                b.set_coulomb_style("ewald")
                with pytest.raises(MMCError, match="MMC_ERR_STATE.*mmc_batch_recip_long"):
                    b.run(n_steps, Q_T, Q_DR, Q_DPHI, seed=9, energies=e0, n_parts=parts, n_threads=2)
                with pytest.raises(MMCError, match="MMC_ERR_STATE.*mmc_batch_recip_long"):
                    b.eval(1, np.tile(a["com"][0], (R8, 1)), np.tile(a["coords"][:3], (R8, 1, 1)))
                with pytest.raises(MMCError, match="MMC_ERR_STATE.*mmc_batch_recip_long"):
                    b.widom(4, Q_T, seed=1)
                b.recip_long()
            b.set_option("trace_steps", n_steps)
            e1, st = b.run(n_steps, Q_T, Q_DR, Q_DPHI, seed=9, energies=e0, n_parts=parts, n_threads=2,
                           replica0=REPLICA0)
            got.append((e1, b.get_trace(n_steps), [b.get_replica(r) for r in range(R8)]))
    (ea, (da, fa), fin_a), (eb, (db, fb), fin_b) = got
    assert np.array_equal(ea.view(np.uint64), eb.view(np.uint64))
    assert np.array_equal(da.view(np.uint64), db.view(np.uint64)) and np.array_equal(fa, fb)
    assert (fa & 1).any() and not (fa & 1).all()
    for r in range(R8):
        for x, y in zip(fin_a[r], fin_b[r]):
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64)), r


def test_potential_ewald_clears_the_stale_mark():
    a = arrays("q216")
    with make_batch(a, 2, Q_RCUT) as b:
        b.set_option("device_moves", 1)
        b.set_coulomb_style("wolf")
        b.run(30, Q_T, Q_DR, Q_DPHI, seed=3, energies=b.potential_wolf(as_array=True)["energy"])
        b.set_coulomb_style("ewald")
        e = b.potential_ewald(as_array=True)["energy"].copy()      # rebuilds S(k) itself
        e1, _ = b.run(30, Q_T, Q_DR, Q_DPHI, seed=4, energies=e)
        e2 = b.potential_ewald(as_array=True)["energy"]
        assert np.abs(e1 - e2).max() < TOL * 1e5


def test_switching_needs_no_outstanding_proposals():
    from metropolismontecarlo_amd._lib import MMCError
    a = arrays("q216")
    with make_batch(a, 2, Q_RCUT) as b:
        b.recip_long()
        b.eval(1, np.tile(a["com"][0], (2, 1)), np.tile(a["coords"][:3], (2, 1, 1)))
        with pytest.raises(MMCError, match="MMC_ERR_STATE"):
            b.set_coulomb_style("wolf")
        assert b.coulomb_style == "ewald"
        b.settle(np.zeros(2, dtype=bool))
        b.set_coulomb_style("wolf")
        with pytest.raises(ValueError):
            b.set_coulomb_style("bare")


# ---- 7: the fences --------------------------------------------------------------------------------
def _ewald_run(b, e0):
    e1, st = b.run(40, Q_T, Q_DR, Q_DPHI, seed=21, energies=e0, n_threads=2)
    return e1, [b.get_replica(r)[1] for r in range(b.R)]


def _fence_cases(box=1.0):
    one = np.ones
    return {
        "set_boxes": (lambda b: b.set_boxes(np.full(b.R, box)), True),
        "kernel=4": (lambda b: b.set_option("kernel", 4), True),
        "persistent=1": (lambda b: b.set_option("persistent", 1), True),
        "volume_change": (lambda b: b.volume_change(box * 1.01, 5.6 / (box * 1.01)), False),
        "volume_trial": (lambda b: b.volume_trial(box * 1.01, 5.6 / (box * 1.01)), False),
        "volume_accept": (lambda b: b.volume_accept(), False),
        "volume_reject": (lambda b: b.volume_reject(), False),
        "volume_trial_replicas": (lambda b: b.volume_trial_replicas(np.full(b.R, box * 1.01)), False),
        "volume_settle": (lambda b: b.volume_settle(one(b.R)), False),
        "run_npt": (lambda b: b.run_npt(1, Q_T, 1.0, 10.0, Q_DR, Q_DPHI, 1, 0.0), False),
        "run_npt_replicas": (lambda b: b.run_npt_replicas(1, Q_T, 1.0, 10.0, Q_DR, Q_DPHI, 1, np.zeros(b.R)), False),
        "widom": (lambda b: b.widom(4, Q_T, seed=1), False),
        "widom_at": (lambda b: b.widom_at(np.zeros((b.R, 2, 12)) + 1.0, Q_T), False),
    }


@pytest.mark.parametrize("name", list(_fence_cases()))
def test_fences(name):
    """Every combination outside the Wolf style's scope returns MMC_ERR_UNSUPPORTED, whichever call
    comes first (where there are two orders: the call is a setting), leaves the style where it was
    and a subsequent Ewald run what it is on a batch that never saw the refused call."""
    from metropolismontecarlo_amd._lib import MMCError
    # (per-replica boxes want kappa sqrt(r_cut^2 + 100) <= 4 at kappa = 5.6 / (2 r_cut): r_cut 10 A, configuration 4)
    a, rcut = (arrays("cfg4"), C4_RCUT) if name == "set_boxes" else (arrays("q216"), Q_RCUT)
    call, is_setting = _fence_cases(a["box"])[name]
    R = 1 if name in ("volume_trial", "volume_accept", "volume_reject", "run_npt") else 2

    def fresh():
        b = make_batch(a, R, rcut)
        b.set_option("device_moves", 1)
        return b, b.potential_ewald(as_array=True)["energy"].copy()

    with fresh()[0] as c:                                   # the control: Ewald, never fenced
        want = _ewald_run(c, c.potential_ewald(as_array=True)["energy"].copy())
    b, e0 = fresh()
    with b:                                                 # Wolf first, then the call
        b.set_coulomb_style("wolf")
        with pytest.raises(MMCError, match="MMC_ERR_UNSUPPORTED"):
            call(b)
        assert b.coulomb_style == "wolf"
        b.set_coulomb_style("ewald")
        b.recip_long()
        got = _ewald_run(b, e0)
        assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)), name
        for x, y in zip(got[1], want[1]):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), name
    if not is_setting:
        return
    with fresh()[0] as c:                                   # the control with the setting alone
        call(c)
        if name == "set_boxes":
            c.recip_long()
        want = _ewald_run(c, c.potential_ewald(as_array=True)["energy"].copy())
    b, _ = fresh()
    with b:                                                 # the setting first, then Wolf
        call(b)
        if name == "set_boxes":
            b.recip_long()
        with pytest.raises(MMCError, match="MMC_ERR_UNSUPPORTED"):
            b.set_coulomb_style("wolf")
        assert b.coulomb_style == "ewald"
        got = _ewald_run(b, b.potential_ewald(as_array=True)["energy"].copy())
        assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)), name
        for x, y in zip(got[1], want[1]):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), name
