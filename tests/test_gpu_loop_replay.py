"""Whole Loop() runs (Ewald/main.jl:487-644) through the reference's call surface (api.py, the
context of csrc/mmc_ctx.inc and its server csrc/mmc_ctxsrv.hpp), each against the oracle stepping
the same chain (tests/loop_replay.py): the chain's own Metropolis decisions and rejections, sweeps
that wrap n_mol -> 1, Adjust!-grown steps, overlaps, scripted edge moves, rebinding, bulk edits,
the "bare" style, systems the server does not take, volume moves and a 10 000-molecule system.

Every call the context answers from state it infers (ctx_sync_call's two molecules, the
look-ahead records of molecule i + 1, the speculative RecipMove and its base buffer) is checked
against the oracle, and every run asserts from Context.stats() that the path it means to test
fired."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import common
import loop_replay as lr
from common import rel
from metropolismontecarlo_amd import api, structs
from metropolismontecarlo_amd.structs import EWALD, Properties

pytestmark = pytest.mark.gpu
TOL = 1e-9
RCUT = lr.RCUT
MODES = ("lookahead", "no_lookahead", "wgs", "launch")


@pytest.fixture(autouse=True)
def _cleanup():
    yield
    api.release_sessions()


@contextmanager
def server_mode(mode):
    """The context's serving form for a whole run: the latency server with look-ahead (default),
    MMC_CTX_LOOKAHEAD=0, the MMC_CTX_WGS server, or launches (set_option("server", 0), applied by
    reference_run once the session exists).  Env vars are read when a server starts, so they hold
    for the run and are cleared after it."""
    env = {"no_lookahead": ("MMC_CTX_LOOKAHEAD", "0"), "wgs": ("MMC_CTX_WGS", "2")}.get(mode)
    api.release_sessions()
    if env:
        os.environ[env[0]] = env[1]
    try:
        yield
    finally:
        if env:
            os.environ.pop(env[0], None)
        api.release_sessions()


def new_ewald(box):
    """main.jl:290-303: a dummy EWALD, then PrepareEwaldVariables."""
    ewald = EWALD(5.6 / box, 5, 27, 1, [[1, 1, 1]] * 3, [0.0, 0.0], np.zeros(2, complex),
                  np.zeros(2, complex), structs.factor)
    return api.PrepareEwaldVariables(ewald, box)


def stats_of(st):
    return st.ewald._session.ctx.stats()


def ewald_checker(lk):
    """Per block: the running energy against potential(..., "ewald") (energy.jl:946-1032) and that
    against the oracle's potential_ewald; the caller's sumQExpOld against the oracle's."""
    def check(st, running, k):
        tot = api.potential(st.moa, st.soa, Properties(), st.ewald, st.vdwTable, st.totProps, "ewald")
        assert rel(running, tot.energy) < TOL, (k, running, tot.energy)
        ref = lk.total()
        assert rel(tot.energy, ref) < TOL, (k, tot.energy, ref)
        lk.check_s_old(st.ewald.sumQExpOld, f"potential() after move {k}")
    return check


def reference_run(a, mode, n_moves, seed=7, order="sweep", script=None, between=None,
                  commit="copy", block=None, adjust_every=50):
    """One Loop() run over the five reference calls in a serving mode; returns (records, stats,
    lockstep, state).  The block checks (potential(), which re-sends the system and stops the
    server) never fall between molecule n_mol and molecule 1 of a sweep, so that a sweep wraps
    on a live context (its look-ahead and unsettled speculative S(k) included)."""
    n_mol = a["com"].shape[0]
    block = block or (2 * n_mol) // 3
    if order == "sweep":
        assert all((m * block) % n_mol for m in range(1, n_moves // block + 1) if m * block < n_moves)
    with server_mode(mode):
        st = lr.LoopState(a, new_ewald(float(a["box"])), seed)
        lk = lr.Lockstep(a)
        total = api.potential(st.moa, st.soa, Properties(), st.ewald, st.vdwTable, st.totProps,
                              "ewald").energy
        assert rel(total, lk.start_total) < TOL
        if mode == "launch":
            st.ewald._session.ctx.set_option("server", 0)
        form = lr.ReferenceForm(api, st, commit=commit)
        _, rec = lr.run(form, st, order, n_moves, lockstep=lk, total=total, script=script,
                        between=between, check_total=ewald_checker(lk),
                        block=block, adjust_every=adjust_every)
        stats = stats_of(st)
    assert lk.checked == n_moves
    return rec, stats, lk, st


def assert_path(mode, stats):
    """The serving path the mode means fired, and no other."""
    if mode == "launch":
        assert stats["launch_evals"] > 0 and stats["cmds"] == 0, stats
        return
    assert stats["cmds"] > 0 and stats["retries"] == 0 and stats["launch_evals"] == 0, stats
    assert stats["spec_hits"] > 0, stats
    if mode == "lookahead":
        assert stats["look_ahead_hits"] > 0, stats
    else:
        assert stats["look_ahead_posted"] == 0, stats


def wrap_probe(n_mol):
    """between-hooks of lr.run that read Context.stats() before molecule n_mol's move, before
    molecule 1's move of the next sweep and after it."""
    wrap = {}

    def at(key):
        def hook(st, e):
            wrap[key] = stats_of(st)
            return e
        return hook
    return wrap, {n_mol - 1: at("before_last"), n_mol: at("before_first"),
                  n_mol + 1: at("after_first")}


def assert_live_wrap(mode, wrap):
    """The sweep wrapped on a live context: no server restart from molecule n_mol's move to the end
    of molecule 1's; on the look-ahead server molecule n_mol's command posted the look-ahead of
    molecule 1 (m2 = (m + 1) % n_mol, mmc_ctx.inc:981), which answered molecule 1's old state
    (:898-941): one command for molecule 1's move, the one for its moved state."""
    b, f, a = wrap["before_last"], wrap["before_first"], wrap["after_first"]
    if mode == "launch":
        assert a["launch_evals"] > b["launch_evals"] and a["cmds"] == 0, wrap
        return
    assert a["launches"] == b["launches"] and a["retries"] == 0, wrap
    if mode == "lookahead":
        assert f["look_ahead_posted"] == b["look_ahead_posted"] + 1, wrap
        assert a["look_ahead_hits"] == f["look_ahead_hits"] + 1, wrap
        assert a["cmds"] == f["cmds"] + 1, wrap
    else:
        assert a["cmds"] == f["cmds"] + 2 and a["look_ahead_posted"] == 0, wrap


@pytest.mark.parametrize("k,variant", [(k, v) for k in (1, 2, 3, 4) for v in ("reference", "unwrapped")])
def test_loop_replay_in_every_serving_mode(k, variant):
    """NVT Ewald Loop() on NIST config k: 2 sweeps (config 4: 1 and 50 moves), dr_max / dphi_max
    adjusted every 50 moves (main.jl:632-638), in the four serving modes.  Pins ctx_sync_call
    (:1107) against the chain's own rejections (main.jl:623-628), the look-ahead (:898-941) over
    a sweep that wraps from molecule n_mol to 1 on a live context (assert_live_wrap), the speculative RecipMove and its base buffer (:960-971, mmc_call_recip_move)
    against Loop()'s array copies (:621,628).  Every call against the oracle; the four modes take
    the same decisions; look-ahead on / off bit for bit; server and launches to 1e-11."""
    a = common.nist_arrays(k, variant)
    n_mol = a["com"].shape[0]
    n_moves = n_mol + 50 if k == 4 else 2 * n_mol
    runs, close = {}, {}
    for mode in MODES:
        wrap, between = wrap_probe(n_mol)
        # molecule n_mol's drawn move is accepted, so that molecule 1 may be answered by look-ahead
        script = {n_mol - 1: dict(accept=True)}
        rec, stats, lk, st = reference_run(a, mode, n_moves, seed=100 + k, script=script,
                                           between=between)
        assert_path(mode, stats)
        assert rec[n_mol - 1][2] and rec[n_mol][0] == 1, rec[n_mol - 1]
        assert_live_wrap(mode, wrap)
        runs[mode], close[mode] = rec, lk.report()
    dec = {m: [(r[0], r[2], r[3]) for r in rec] for m, rec in runs.items()}
    for m in MODES[1:]:
        assert dec[m] == dec["lookahead"], (m, close)
    acc = np.mean([d[1] for d in dec["lookahead"]])
    assert 0.2 < acc < 0.9, acc
    v = {m: np.array([r[4] for r in rec]) for m, rec in runs.items()}
    assert np.array_equal(v["lookahead"], v["no_lookahead"])
    for m in ("wgs", "launch"):   # the calls' own results (delta, their difference, is derived)
        err = np.abs(v[m] - v["lookahead"])[:, :-1] / np.maximum(np.abs(v["lookahead"][:, :-1]), 1.0)
        assert err.max() < 1e-11, (m, err.max(), np.unravel_index(err.argmax(), err.shape))


@pytest.mark.parametrize("order", ["random", "twice"])
def test_loop_replay_out_of_sweep_order(order):
    """Loop() bodies whose next molecule is not i + 1: random molecules and each molecule twice in
    a row.  The look-ahead of molecule i + 1 must not answer another molecule, and a repeated
    molecule's old state is the state its own previous move left (ctx_sync_call, :1107-1117)."""
    a = common.nist_arrays(2, "unwrapped")
    rec, stats, lk, _ = reference_run(a, "lookahead", 300, seed=31, order=order, block=150)
    assert stats["retries"] == 0 and stats["spec_hits"] > 0 and stats["cmds"] > 0


def test_loop_replay_scripted_edges():
    """Config 2 (unwrapped), 1.5 sweeps on the latency server with scripted events, every call
    against the oracle:
    * overlaps (ewalds.jl:359) on molecule 11, the move before the look-ahead molecule 12, and on
      molecule 200, the last of the sweep (look-ahead wraps to 1): RecipMove is skipped
      (main.jl:580) and the speculative S(k) of the command is left unsettled for molecule 1's
      move, on the same server launch (no block check falls on the wrap);
    * zero-displacement moves rejected and accepted (sumQExpNew == sumQExpOld bit for bit, which
      defeats finding the base buffer by content, mmc_call_recip_move :1243-1254);
    * Julia-style rebinding mid-run: new moa.COM / soa.coords array objects, and RecipCommit /
      RecipRollback instead of the copies for a stretch of moves;
    * a bulk edit of 40 molecules followed by sync_system (api.py), with S(k) brought along by a
      RecipMove per edited molecule.
    Run on the latency server and on launches."""
    a = common.nist_arrays(2, "unwrapped")
    results = {}
    for mode in ("lookahead", "launch"):
        script = {}

        def scripted(k, make):
            def hook(st, e):
                script[k] = make(st)
                return e
            return hook

        def rebind(st, e):
            st.moa.COM = st.moa.COM.copy()
            st.soa.coords = st.soa.coords.copy()
            forms[0].commit = "api"
            return e

        def unbind(st, e):
            forms[0].commit = "copy"
            return e

        def bulk_edit(st, e):
            rng = np.random.default_rng(99)
            lk = locks[0]
            before = lk.total()
            lk.check_s_old(st.ewald.sumQExpOld, "before the bulk edit")
            for m in rng.choice(np.arange(1, 201), size=40, replace=False):
                m = int(m)
                d = (rng.random(3) - 0.5) * 0.4
                f, l = st.span(m)
                ra_old = st.atoms(m)
                st.place(m, st.moa.COM[m - 1] + d, ra_old + d)
                lk.s.com[m - 1], lk.s.coords[f:l] = st.moa.COM[m - 1], st.soa.coords[f:l]
                _, st.ewald = api.RecipMove(st.box, st.ewald, ra_old, ra_old + d, st.soa.charge[f:l])
                st.ewald.sumQExpOld = st.ewald.sumQExpNew.copy()
            api.sync_system(st.moa, st.soa)
            after = lk.total()
            lk.check_s_old(st.ewald.sumQExpOld, "after the bulk edit")
            return e + (after - before)

        forms, locks = [], []
        wrap, between = wrap_probe(200)
        between.update({10: scripted(10, lambda st: lr.overlap_move(st, 11)),
                   40: scripted(40, lambda st: lr.zero_move(st, 41, False)),
                   41: scripted(41, lambda st: lr.zero_move(st, 42, True)),
                   60: scripted(60, lambda st: lr.zero_move(st, 61, True)),
                   80: rebind, 140: unbind, 230: bulk_edit})
        probe_last, overlap_last = between[199], scripted(199, lambda st: lr.overlap_move(st, 200))
        between[199] = lambda st, e: overlap_last(st, probe_last(st, e))
        with server_mode(mode):
            st = lr.LoopState(a, new_ewald(float(a["box"])), 5)
            lk = lr.Lockstep(a)
            locks.append(lk)
            total = api.potential(st.moa, st.soa, Properties(), st.ewald, st.vdwTable,
                                  st.totProps, "ewald").energy
            if mode == "launch":
                st.ewald._session.ctx.set_option("server", 0)
            forms.append(lr.ReferenceForm(api, st))
            _, rec = lr.run(forms[0], st, "sweep", 300, lockstep=lk, total=total, script=script,
                            between=between, check_total=ewald_checker(lk), block=130)
            stats = stats_of(st)
        assert_path(mode, stats)
        b, f, w = wrap["before_last"], wrap["before_first"], wrap["after_first"]
        if mode == "launch":
            assert w["cmds"] == 0 and w["launch_evals"] > b["launch_evals"], wrap
        else:   # overlap on 200, rejected: look-ahead posted but refused; molecule 1 on its own
            assert w["launches"] == b["launches"] and w["retries"] == 0, wrap
            assert f["look_ahead_posted"] == b["look_ahead_posted"] + 1, wrap
            assert w["look_ahead_hits"] == f["look_ahead_hits"] and w["cmds"] == f["cmds"] + 2, wrap
        assert rec[10][3] and rec[199][3] and not rec[10][2] and not rec[199][2]
        assert not rec[40][2] and rec[41][2] and rec[60][2]
        assert lk.checked == 300
        results[mode] = rec
    assert [r[:4] for r in results["lookahead"]] == [r[:4] for r in results["launch"]]


def test_loop_replay_bare_style():
    """coulombStyle "bare" (main.jl:494-499,560-565): LJ_poly_dU(i, system) (energy.jl:126-206) and
    CoulombReal (energy.jl:618-711) per move, no RecipMove, on config 1 with a scripted overlap
    (energy.jl:695).  Every call against orc.coulomb_real; the LJ evaluations by launch
    (Context.stats()); the running energy against the sum the
    moves add up; the Wolf totals of potential() (energy.jl:864-943) against orc.potential_wolf."""
    a = common.nist_arrays(1, "reference")
    api.release_sessions()
    st = lr.LoopState(a, new_ewald(float(a["box"])), 23)
    lk = lr.Lockstep(a, "bare")
    total = lk.start_total

    def check(st, running, k):
        assert rel(running, lk.total()) < TOL, k
        w = api.potential(st.moa, st.soa, Properties(), st.ewald, st.vdwTable, st.totProps)
        wo = lk.orc.potential_wolf(lk.s, lk.ew, RCUT, RCUT, literal_prefactor=False)
        assert rel(w.energy, wo["energy"]) < TOL and rel(w.coulomb, wo["coulomb"]) < TOL, k

    script = {}
    between = {30: lambda st, e: script.__setitem__(30, lr.overlap_move(st, 31)) or e}
    _, rec = lr.run(lr.ReferenceForm(api, st, "bare"), st, "sweep", 150, lockstep=lk, total=total,
                    script=script, between=between, check_total=check, block=50)
    assert rec[30][3] and not rec[30][2]
    assert 0.2 < np.mean([r[2] for r in rec]) < 0.95
    assert lk.checked == 150
    # the Requirements forms re-send the system and evaluate by launch: no EWALD on that session,
    # so the server does not apply (ctx_server_applies, :257)
    ctx = api._sessions[id(st.system._mmc_cache[1])].ctx
    stats = ctx.stats()
    assert stats["cmds"] == 0 and stats["launch_evals"] >= 2 * 150 - 1, stats


@pytest.mark.parametrize("system", ["mea_tip3p", "ragged"])
def test_loop_replay_where_the_server_does_not_apply(system):
    """Systems ctx_server_applies (:257) turns away -- the MEA/TIP3P deck (11-atom MEAs among
    waters) and a ragged random system -- run the whole Loop() on launches.  Loop() moves the
    3-site molecules only (RecipMove's n == 3, ewalds.jl:740)."""
    if system == "mea_tip3p":
        a = common.mea_tip3p_box()
    else:
        a = common.random_system(120, 24.0, seed=4, na_choices=(2, 3, 4))
    na = a["last_atom"] - a["first_atom"] + 1
    movable = [int(m) + 1 for m in np.nonzero(na == 3)[0]]
    n_moves = min(2 * len(movable), 300)
    rec, stats, lk, _ = reference_run(a, "lookahead", n_moves, seed=8, order=movable, block=150)
    assert stats["cmds"] == 0 and stats["launch_evals"] > 0, stats
    assert any(r[2] for r in rec) and not all(r[2] for r in rec)


def test_loop_replay_with_volume_moves():
    """Per-move calls around NPT volume moves at the Context level (npt.VolumeChange's device calls,
    volumeChange.jl:59-147): a sweep of trial_move / accept_move / reject_move, a volume move
    forced to reject, half a sweep, a volume move forced to accept, after which the caller
    refreshes its arrays from download_system and goes on in the new box and kappa.  The first
    per-move calls after the accept must match the oracle in the rescaled system: they exercise
    ctx_mirror_catch_up (:451) and the server restart on a new box / kappa (:944-947)."""
    from metropolismontecarlo_amd.device import Context
    a = common.nist_arrays(2, "unwrapped")
    box0 = float(a["box"])
    with Context() as ctx:
        ctx.upload_system(a["com"], a["first_atom"], a["last_atom"], a["coords"], a["atype"],
                          a["charge"], a["eps"], a["sig"], box0)
        ctx.prepare_ewald(5.6 / box0, 5, 27, box0, structs.factor)
        st = lr.LoopState(a, None, 41)
        lk = lr.Lockstep(a)
        running = ctx.potential_ewald(RCUT, RCUT)["energy"]
        assert rel(running, lk.start_total) < TOL
        form = lr.TrialForm(ctx, st)

        def check(st, e, k):
            assert rel(e, ctx.potential_ewald(RCUT, RCUT)["energy"]) < TOL, k
            assert rel(e, lk.total()) < TOL, k

        running, _ = lr.run(form, st, "sweep", 200, lockstep=lk, total=running, check_total=check)
        s0 = ctx.stats()
        # rejected volume move: the trial's totals at the new volume, then nothing changed
        tot = ctx.volume_trial(box0 * 1.015, 5.6 / (box0 * 1.015), RCUT, RCUT)
        sc = lk.s.copy()
        f = box0 * 1.015 / box0
        for j in range(sc.n_mol):
            for d in range(3):
                old = sc.com[j, d]
                nw = old * f
                sc.com[j, d] = nw
                sc.coords[3 * j:3 * j + 3, d] += nw - old
        sc.box = box0 * 1.015
        ew_t = lk.orc.Ewald(5.6 / sc.box, 5, 27, sc.box, factor=structs.factor)
        assert rel(tot["energy"], lk.orc.potential_ewald(sc, ew_t, RCUT, RCUT)["energy"]) < TOL
        ctx.volume_reject()
        running, _ = lr.run(form, st, "sweep", 100, lockstep=lk, total=running, check_total=check)
        # accepted volume move
        box1 = box0 * 1.01
        tot = ctx.volume_trial(box1, 5.6 / box1, RCUT, RCUT)
        ctx.volume_accept()
        com, coords = ctx.download_system()
        f = box1 / box0
        want_com = lk.s.com * f
        assert np.abs(com - want_com).max() < 1e-12 * box1
        st.moa.COM[...] = com
        st.soa.coords[...] = coords
        st.box = st.totProps.box = box1
        lk.s.com[...], lk.s.coords[...], lk.s.box = com, coords, box1
        lk.ew = lk.orc.Ewald(5.6 / box1, 5, 27, box1, factor=structs.factor)
        running = tot["energy"]
        assert rel(running, lk.total()) < TOL
        # the first per-molecule calls in the new box, then trial moves from molecule 101 on
        for i in (101, 102):
            p, v = ctx.lj_poly_du(i, RCUT)
            e, _, ov = ctx.ewald_short(i, RCUT)
            po, vo = lk.orc.lj_poly_du(i, lk.s, RCUT)
            eo, _, ovo = lk.orc.ewald_short(i, lk.s, lk.ew, RCUT)
            assert ov == ovo and rel(p, po) < TOL and rel(v, vo, abs(po)) < TOL and rel(e, eo) < TOL
        running, rec = lr.run(form, st, [*range(101, 201), *range(1, 101)], 200, lockstep=lk,
                              total=running, check_total=check)
        s1 = ctx.stats()
        assert s1["cmds"] > s0["cmds"] and s1["launches"] > s0["launches"] and s1["retries"] == 0
        assert any(r[2] for r in rec)


def test_loop_replay_at_10000_molecules():
    """500 consecutive moves of one sweep on the 10 000-molecule SPC/E lattice of
    test_gpu_at_size.py, through the five reference calls on the latency server in its
    large-system shape (21 workgroups, :290-297), look-ahead and speculative RecipMove included."""
    from test_gpu_npt import water_lattice
    a = water_lattice(10000, "spce")
    rec, stats, lk, _ = reference_run(a, "lookahead", 500, seed=3, block=500)
    assert_path("lookahead", stats)
    assert any(r[2] for r in rec) and not all(r[2] for r in rec)
