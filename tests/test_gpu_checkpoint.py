"""Save and resume on the GPU: a batch that is saved, destroyed, created anew from OTHER coordinates
and loaded continues every chain bit for bit, on every run path; load restores every layout the
kernels read; record ranges; refusals that leave the batch untouched.

Every comparison is bitwise (tobytes() / integer equality): there is no tolerance in this file.
NIST configuration 1 (100 molecules, L = 20 A, r_cut 10 A) with R = 24 unless a case says otherwise.

Not here: recovery from a failed run through set_state.  The torn-record test hook (option
"inject_torn") makes the driver read a record again and the run succeed; no hook leaves the batch in
the state that needs every replica set again, and a test may not provoke a device fault to get there."""
import numpy as np
import pytest

import common
import test_gpu_moves as gm
from metropolismontecarlo_amd import _lib, checkpoint, moves, structs
from metropolismontecarlo_amd._lib import MMCError
from metropolismontecarlo_amd.device import Batch

pytestmark = pytest.mark.gpu

R = 24
T, DR, DPHI = 298.15, 0.316555789, 0.05
SEED, REPLICA0 = 20261020, 3000
COUNTS = ("moves", "trans_attempt", "trans_accept", "rot_attempt", "rot_accept", "overlaps")
SHIFT = np.array([3.7, -11.3, 26.9])
TRACE = 20


def shifted(a):
    """The configuration moved by a constant vector, molecules re-wrapped by their centres of mass."""
    com = a["com"] + SHIFT
    w = np.floor(com / a["box"]) * a["box"]
    return dict(a, com=com - w, coords=a["coords"] + SHIFT - np.repeat(w, 3, axis=0))


def make(a, n_rep=R, rcut=10.0, options=None, chunk=5):
    b = Batch(n_rep, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"], 5.6 / a["box"],
              structs.factor, rcut, rcut)
    for k, v in (options or {}).items():
        b.set_option(k, v)
    b.set_option("state_chunk", chunk)            # five chunks of R = 24, the last one ragged, both staging buffers
    return b


def bits(x):
    return np.ascontiguousarray(x).tobytes()


def counts(st):
    return [int(st[k]) for k in COUNTS]


def device_order(s_ref, info):
    """get_replica's S(k) (the reference's k-vector walk, ewalds.jl:57-89: kx = 0..nk, ky and kz =
    -nk..nk, 0 < k^2 < k_sq_max) in the order a record holds it (include/mmc_hip.h, "Save and
    resume"): the same walk with, on a half_k batch, the later member of each kx = 0 conjugate pair
    left out.  The entries that stay are copies, so the comparison with a record is bitwise."""
    d = checkpoint.info_to_dict(info)
    nk, k_sq_max, half_k = min(int(d["nk"]), 5), int(d["k_sq_max"]), bool(d["half_k"])
    keep = [not (half_k and kx == 0 and (ky > 0 or (ky == 0 and kz > 0)))
            for kx in range(nk + 1) for ky in range(-nk, nk + 1) for kz in range(-nk, nk + 1)
            if 0 < kx * kx + ky * ky + kz * kz < k_sq_max]
    assert len(keep) == s_ref.shape[0] and sum(keep) == int(d["nkvecs"]), (len(keep), sum(keep), s_ref.shape)
    return s_ref[np.array(keep)]


# ---- the run paths ------------------------------------------------------------------------------------
class Path:
    """One way of driving a batch.  configure(): the modes a fresh batch is put into (arm A; load does
    it in arm B).  start(): the caller's arrays.  leg(): one leg, updates them, returns its counts.
    observe(): what the path adds to the comparison."""
    n_rep, rcut, options, config, variant = R, 10.0, {}, 1, "unwrapped"
    trace = TRACE            # option "trace_steps" of leg 2 (0: a launch of several steps records no single steps)
    n1 = n2 = 2 * 100 + 7
    kw = dict(n_groups=2, n_threads=2, replica0=REPLICA0)

    def arrays(self):
        return common.nist_arrays(self.config, self.variant)

    def configure(self, b):
        pass

    def total(self, b):
        return b.potential_ewald(as_array=True)

    def start(self, b):
        return dict(energies=self.total(b)["energy"].copy())

    def leg(self, b, c, k):
        c["energies"], st = b.run(self.n2 if k else self.n1, T, DR, DPHI, SEED, energies=c["energies"], **self.kw)
        self.check_stats(st, self.n2 if k else self.n1)
        return counts(st)

    def check_stats(self, st, n):
        pass

    def observe(self, b):
        return {}


class Headline(Path):
    """The headline form.  The driver takes several steps per launch only while no trace of single steps
    is asked for (run_plan, mmc_engine.inc), so this path and WholeCall leave the trace off -- their
    launch counts show the form -- and HeadlineTraced compares the trace of the same options."""
    options = dict(device_moves=1, kernel=2, persistent=0, accept_on_device=1, steps_per_launch=8)
    n1 = n2 = 20
    trace = 0
    kw = dict(Path.kw, n_parts=1)

    def check_stats(self, st, n):
        assert st["device_decisions"] == self.n_rep * n and st["launches"] == 2 * 3, st      # 8 + 8 + 4


class WholeCall(Headline):
    options = dict(Headline.options, whole_call=1)

    def check_stats(self, st, n):
        assert st["device_decisions"] == self.n_rep * n and st["launches"] == 2, st


class HeadlineTraced(Headline):
    trace = TRACE

    def check_stats(self, st, n):
        assert st["device_decisions"] == self.n_rep * n, st


class Server(Path):
    n_rep = 4
    options = dict(device_moves=1, kernel=2, persistent=1)
    n1, n2 = 60, 37
    kw = dict(n_groups=2, n_threads=2, replica0=REPLICA0, n_parts=3)     # (a wave per 64 molecules and one more)

    def check_stats(self, st, n):
        assert st["server_steps"] == n, st


class Chains(Path):
    options = dict(device_moves=1)
    n1 = n2 = 150

    def start(self, b):
        t = self.total(b)
        return dict(chains=b.new_chains(t["energy"], t["virial"], dr_max=DR, dphi_max=DPHI))

    def leg(self, b, c, k):
        return counts(b.run_chains(c["chains"], self.n1, T, SEED, adjust=True, **self.kw))


class Exchange(Path):
    n_rungs, n_rounds, per_round = 6, 3, 25
    options = dict(device_moves=1)

    def configure(self, b):
        b.set_temperatures(np.tile(moves.geometric_ladder(270.0, 420.0, self.n_rungs), R // self.n_rungs))

    def start(self, b):
        return dict(energies=self.total(b)["energy"].copy(), rung=np.tile(np.arange(self.n_rungs, dtype=np.int32), 4),
                    attempt=np.zeros(self.n_rungs - 1, dtype=np.int64), accept=np.zeros(self.n_rungs - 1, dtype=np.int64),
                    round=np.array(0, dtype=np.int64))

    def leg(self, b, c, k):
        c["energies"], st, _, _ = b.run_exchange(self.n_rounds, self.per_round, DR, DPHI, SEED, c["energies"], c["rung"],
                                                 self.n_rungs, round0=int(c["round"]), attempt=c["attempt"],
                                                 accept=c["accept"], **self.kw)
        c["round"] = np.array(int(c["round"]) + self.n_rounds, dtype=np.int64)
        return counts(st)

    def observe(self, b):
        return dict(temperatures=b.temperatures())


class PerBox(Path):
    n_rungs = 6

    def configure(self, b):
        b.set_boxes(20.0 + 0.04 * np.arange(R), 5.6)
        b.set_temperatures(np.tile(moves.geometric_ladder(280.0, 360.0, self.n_rungs), R // self.n_rungs))

    def start(self, b):
        return dict(energies=self.total(b)["energy"].copy(), rung=np.tile(np.arange(self.n_rungs, dtype=np.int32), 4),
                    attempt=np.zeros(self.n_rungs - 1, dtype=np.int64), accept=np.zeros(self.n_rungs - 1, dtype=np.int64),
                    round=np.array(0, dtype=np.int64), vol_accept=np.zeros(R, dtype=np.int64))

    def leg(self, b, c, k):
        c["energies"], st, ns = b.run_npt_replicas(2, T, 0.02, 0.02 * 20.0 ** 3, DR, DPHI, SEED, c["energies"],
                                                   moves_per_sweep=40, n_threads=2, replica0=REPLICA0)
        c["vol_accept"] = c["vol_accept"] + np.array([x["vol_accept"] for x in ns], dtype=np.int64)
        b.exchange(self.n_rungs, c["energies"], c["rung"], SEED, int(c["round"]), pressure=0.02, replica0=REPLICA0,
                   attempt=c["attempt"], accept=c["accept"])
        c["round"] = np.array(int(c["round"]) + 1, dtype=np.int64)
        return counts(st)

    def observe(self, b):
        return dict(boxes=b.get_boxes(), temperatures=b.temperatures())


class Wolf(Path):
    def configure(self, b):
        b.recip_long()
        b.set_coulomb_style("wolf")

    def total(self, b):
        return b.potential_wolf(as_array=True)


class Quaternions(Path):
    rcut, n1, n2 = 9.0, 120, 120
    options = dict(device_moves=1)

    def __init__(self, faithful):
        self.faithful = faithful

    def arrays(self):
        return gm.quaternion_system(216, self.faithful)[0]

    def configure(self, b):
        _, quat, db = gm.quaternion_system(216, self.faithful)
        b.set_orientations(quat, db, faithful=self.faithful)

    def observe(self, b):
        return dict(quat=np.stack([b.get_orientations(r) for r in range(b.R)]))


class Npt(Path):
    """A one-replica NPT chain (its own case beyond these replica counts).  r_cut 9 A, so that the
    box may shrink as well as grow."""
    n_rep, rcut = 1, 9.0
    seed = 31337

    def start(self, b):
        return dict(energies=self.total(b)["energy"].copy(), vol_accept=np.zeros(1, dtype=np.int64))

    def leg(self, b, c, k):
        e, st, ns = b.run_npt(4, T, 0.03, 0.03 * 20.0 ** 3, DR, DPHI, self.seed, float(c["energies"][0]),
                              moves_per_sweep=45, replica0=REPLICA0)
        c["energies"] = np.array([e])
        c["vol_accept"] = c["vol_accept"] + ns["vol_accept"]
        if k == 0:
            assert ns["vol_accept"] > 0, "leg 1 must accept a volume move: choose another seed"
        return counts(st) + [int(ns["vol_attempt"]), int(ns["vol_accept"])]

    def observe(self, b):
        info = b.state_info()
        return dict(box=np.array([info.box, info.kappa, b.box, b.kappa]))


class CandidateLists(Path):
    config = 4
    options = dict(device_moves=1, kernel=2, persistent=0, candidate_lists=1, wave_wgs=1)
    n1 = n2 = 60
    kw = dict(Path.kw, n_parts=1)

    def observe(self, b):
        return dict(cand_state=np.array(b.cand_stats()["state"]))


class Mixture(Path):
    """An SPC/E + TIP3P mixture: no record lines, so get_state and set_state take the array forms
    k_state_pack<false> / k_state_unpack<false>, and the generic move kernel, the only one a
    mixture runs on, reads what they wrote."""
    options = dict(kernel=0)

    def arrays(self):
        return common.spce_tip3p_mixture(1, "interleaved")[0]


class Generic(Path):
    """The generic kernel on a homogeneous system: set_state writes the record lines too, the move
    kernel reads the arrays."""
    options = dict(kernel=0)


class LatencyServer(Path):
    """What a one-replica batch gets from kernel 3 with the server on: the latency server, several
    workgroups a replica, each with its own copy of its molecules, which set_state has to
    invalidate.  (The run statistics tell a server from launches; that the server of one replica
    of 100 molecules is the latency form is run_plan's rule, batch_lat_shape.)"""
    n_rep = 1
    options = dict(device_moves=1, kernel=3, persistent=1)
    n1, n2 = 60, 37
    kw = dict(n_groups=1, n_threads=1, replica0=REPLICA0)

    def check_stats(self, st, n):
        assert st["server_steps"] == n and st["device_decisions"] == 0, st


class LatencySteps(Path):
    """k_move_eval_lat launched per step: kernel 4 with sixteen parts (four workgroups a replica),
    the host adding up and deciding."""
    options = dict(device_moves=1, kernel=4, persistent=0)
    n1, n2 = 60, 37
    kw = dict(Path.kw, n_parts=16)

    def check_stats(self, st, n):
        assert st["server_steps"] == 0 and st["device_decisions"] == 0 and st["launches"] == 2 * n, st
        assert st["moves"] == self.n_rep * n, st


PATHS = {"default": Path(), "headline": Headline(), "whole_call": WholeCall(), "headline_traced": HeadlineTraced(),
         "server": Server(), "chains": Chains(),
         "exchange": Exchange(), "per_box": PerBox(), "wolf": Wolf(), "quat_faithful": Quaternions(True),
         "quat_at": Quaternions(False), "npt": Npt(), "cand_lists": CandidateLists(),
         "mixture": Mixture(), "generic": Generic(), "latency_server": LatencyServer(),
         "latency_steps": LatencySteps()}


def arm(path, interrupted, ckpt):
    a = path.arrays()
    b = make(a, path.n_rep, path.rcut, path.options)
    try:
        path.configure(b)
        c = path.start(b)
        first = path.leg(b, c, 0)
        listed = None
        if interrupted:
            b.save(ckpt, extra=c)
            b.close()
            b = make(shifted(a), path.n_rep, path.rcut, path.options)      # options are the caller's; modes are load's
            c = b.load(ckpt)
            listed = b.cand_stats()["list_steps"]
        b.set_option("trace_steps", path.trace)
        second = path.leg(b, c, 1)
        out = dict(c, records=b.get_state(), first=np.array(first), second=np.array(second))
        du, fl = b.get_trace(path.trace)
        out.update(trace_du=du, trace_flags=fl, **path.observe(b))
        if listed is not None:
            out["list_steps_in_leg_2"] = np.array(b.cand_stats()["list_steps"] - listed)
        return out
    finally:
        b.close()


@pytest.mark.parametrize("name", list(PATHS))
def test_an_interrupted_run_continues_bit_for_bit(name, tmp_path):
    path = PATHS[name]
    whole = arm(path, False, None)
    resumed = arm(path, True, str(tmp_path / "run.ckpt"))
    grown = resumed.pop("list_steps_in_leg_2")
    assert sorted(whole) == sorted(resumed)
    for k in whole:
        x, y = np.asarray(whole[k]), np.asarray(resumed[k])
        assert x.dtype == y.dtype and x.shape == y.shape, k
        if x.dtype.names:                                    # the mmc_chain array, field by field
            for f in x.dtype.names:
                assert bits(x[f]) == bits(y[f]), (k, f)
        assert bits(x) == bits(y), k
    assert whole["second"][2] + whole["second"][4] > 0                            # leg 2 accepted moves
    if path.trace:
        assert np.any(whole["trace_flags"] & 1) and np.any(whole["trace_du"] != 0.0)
    if name == "cand_lists":
        assert int(whole["cand_state"]) == 1 and int(grown) > 0        # rebuilt and used after load


# ---- every layout is restored ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """A batch after a leg of the headline form (the saver, kept open and left alone: no test may
    rebuild its S(k)), its checkpoint, a fresh batch from other coordinates that has loaded it, and
    the totals of the saved state from a third batch that ran the same leg."""
    a = common.nist_arrays(1, "unwrapped")
    path = str(tmp_path_factory.mktemp("ckpt") / "saved.ckpt")

    def after_the_leg():
        b = make(a, options=Headline.options)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        e, _ = b.run(40, T, DR, DPHI, SEED, energies=e, n_groups=2, n_threads=2, n_parts=1, replica0=REPLICA0)
        return b, e
    b, e = after_the_leg()
    b.save(path, extra=dict(energies=e), replica0=REPLICA0)
    with after_the_leg()[0] as twin:                           # (potential_ewald replaces S(k) by a fresh sum)
        assert bits(twin.get_state()) == bits(b.get_state())
        totals = twin.potential_ewald(as_array=True).copy()
    fresh = make(shifted(a), options=Headline.options)
    extra = fresh.load(path)
    yield dict(a=a, b=b, fresh=fresh, path=path, e=e, extra=extra, totals=totals)
    b.close()
    fresh.close()


def test_load_restores_every_layout(saved):
    b, f = saved["b"], saved["fresh"]
    assert bits(saved["extra"]["energies"]) == bits(saved["e"])
    assert bits(f.get_state()) == bits(b.get_state())
    for r in (0, R // 2, R - 1):                                              # the SoA path
        for x, y in zip(b.get_replica(r), f.get_replica(r)):
            assert bits(x) == bits(y), r
    assert bits(b.rdf_sites(50, per_replica=True)) == bits(f.rdf_sites(50, per_replica=True))   # records / LDS staging
    lo_b, lo_f = b.local_order(per_replica=True, details=True), f.local_order(per_replica=True, details=True)
    assert sorted(lo_b) == sorted(lo_f)
    for k in lo_b:
        assert bits(lo_b[k]) == bits(lo_f[k]), k
    # widom reads S(k) without rebuilding it: a wrong S buffer shows.  Before potential_ewald, which rebuilds it.
    w_b = b.widom(8, T, 77, offsets=b.widom_offsets, outputs=True)
    w_f = f.widom(8, T, 77, offsets=b.widom_offsets, outputs=True)
    assert len(w_b) == len(w_f) == 5                                          # sums, counts, mol, du, ovl
    for x, y in zip(w_b, w_f):
        assert bits(x) == bits(y)
    assert np.any(w_b[3][:, :, 2] != 0.0)                                     # the reciprocal terms are there
    assert bits(f.potential_ewald(as_array=True)) == bits(saved["totals"])          # (last: it rebuilds f's S(k))


def test_the_file_reads_back_without_a_device(saved):
    head = checkpoint.read_header(saved["path"])
    assert head["replica0"] == REPLICA0 and head["n_records"] == R and head["info"]["steps_done"] == 40
    assert checkpoint.info_to_dict(saved["b"].state_info()) == head["info"]
    for r in (0, 7, R - 1):
        rec = checkpoint.read_replica(saved["path"], r)
        com, coords, s_ref = saved["b"].get_replica(r)
        assert bits(rec["com"]) == bits(com) and bits(rec["coords"]) == bits(coords)
        assert rec["box"] == 20.0 and rec["temperature"] == 0.0 and rec["quat"] is None and rec["flags"] == 0
        # S in device order, entry for entry: get_replica's 337 through the walk the library documents
        assert rec["S"].shape == (head["info"]["nkvecs"],)
        assert bits(rec["S"]) == bits(device_order(s_ref, head["info"]))


# ---- ranges ---------------------------------------------------------------------------------------------
def test_ranges_concatenate_to_the_whole(saved):
    b = saved["b"]
    whole = b.get_state()
    assert whole.shape == (R, checkpoint.record_layout(b.state_info())[1])
    for cuts in ((0, 1, 2, 13, 24), (0, 5, 12, 24), (0, 24), (0, 23, 24)):
        parts = [b.get_state(lo, hi - lo) for lo, hi in zip(cuts, cuts[1:])]
        assert bits(np.concatenate(parts)) == bits(whole), cuts
    assert b.get_state(7, 0).shape[0] == 0
    out = np.zeros((3, whole.shape[1]), dtype=np.uint8)
    assert b.get_state(4, 3, out=out) is out and bits(out) == bits(whole[4:7])
    for opt in (1, 0, -1):                               # both deliveries of the pack kernel give the same bytes
        b.set_option("state_delivery", opt)
        assert bits(b.get_state()) == bits(whole)
    pad = checkpoint.record_layout(b.state_info())[0]
    assert not whole[:, pad[7]:].any() and not whole[:, pad[2] + 8:pad[3]].any()        # padding is zero


@pytest.mark.parametrize("delivery", (0, 1))
def test_set_state_of_a_range_leaves_the_others(saved, delivery):
    a, src = saved["a"], saved["b"]
    with make(shifted(a), options=Headline.options) as dst:
        dst.set_option("state_delivery", delivery)
        e = dst.potential_ewald(as_array=True)["energy"].copy()
        dst.run(8, T, DR, DPHI, SEED + 1, energies=e, n_groups=2, n_threads=2, n_parts=1)   # (S buffers of both parities)
        before = dst.get_state()
        rec = src.get_state(5, 7)
        dst.set_state(src.state_info(), rec, r0=5)
        after = dst.get_state()
        assert bits(after[5:12]) == bits(rec)
        assert bits(after[:5]) == bits(before[:5]) and bits(after[12:]) == bits(before[12:])
        assert bits(before[5:12]) != bits(rec)
        for r in (4, 5, 11, 12):                         # and the layouts behind the records
            want = (src if 5 <= r < 12 else None)
            got = dst.get_replica(r)
            if want is not None:
                for x, y in zip(want.get_replica(r), got):
                    assert bits(x) == bits(y), r
        assert dst.state_info().steps_done == 40
        assert bits(dst.potential_ewald(as_array=True)[5:12]) == bits(saved["totals"][5:12])


# ---- refusals leave the batch untouched -----------------------------------------------------------------
def refused(b, status, call):
    before = b.get_state()
    with pytest.raises(MMCError) as e:
        call()
    assert e.value.status == status, e.value
    assert bits(b.get_state()) == bits(before)


def test_refusals_leave_the_batch_untouched(saved):
    a, b = saved["a"], saved["b"]
    info, rec = b.state_info(), b.get_state()
    a2 = common.nist_arrays(2, "unwrapped")
    with make(a2, 3) as other:                                             # records of a 200-molecule batch
        refused(b, _lib.MMC_ERR_ARG, lambda: b.set_state(other.state_info(), other.get_state(), 0))
    with make(a, options=dict(device_moves=1)) as pb:                      # per-replica records into a one-box batch
        pb.set_boxes(np.full(R, 20.5))
        pb.recip_long()
        refused(b, _lib.MMC_ERR_STATE, lambda: b.set_state(pb.state_info(), pb.get_state(), 0))
        refused(pb, _lib.MMC_ERR_STATE, lambda: pb.set_state(info, rec, 0))
    aq, quat, db = gm.quaternion_system(216, True)
    with make(aq, 3, 9.0, dict(device_moves=1)) as q0, make(aq, 3, 9.0, dict(device_moves=1)) as q1:
        q1.set_orientations(quat, db, faithful=True)                       # quaternion records into mode 0
        refused(q0, _lib.MMC_ERR_STATE, lambda: q0.set_state(q1.state_info(), q1.get_state(), 0))
        assert q1.get_state().shape[1] > q0.get_state().shape[1]
    changed = _lib.StateInfo.from_buffer_copy(info)
    changed.topology ^= 1
    refused(b, _lib.MMC_ERR_ARG, lambda: b.set_state(changed, rec, 0))
    changed = _lib.StateInfo.from_buffer_copy(info)
    changed.temps_on = 1
    refused(b, _lib.MMC_ERR_STATE, lambda: b.set_state(changed, rec, 0))
    bad = rec.copy()                                                       # a record whose box is not the batch's
    off = checkpoint.record_layout(info)[0]
    bad[R - 1, off[0]:off[0] + 8] = np.array([21.0]).view(np.uint8)
    refused(b, _lib.MMC_ERR_ARG, lambda: b.set_state(info, bad, 0))
    with pytest.raises(MMCError) as e:                                      # a range past the last replica, at the library
        _lib.check(b._L.mmc_batch_get_state(b._h, 20, 5, rec.ctypes.data_as(_lib.C.c_void_p)))
    assert e.value.status == _lib.MMC_ERR_ARG


def test_open_moves_refuse_both_calls():
    a = common.nist_arrays(1, "unwrapped")
    with make(a, 2) as b:
        info, rec = b.state_info(), b.get_state()
        com, coords, _ = b.get_replica(0)
        b.eval(np.array([1, 1]), np.stack([com[0]] * 2) + 0.01, np.stack([coords[:3]] * 2) + 0.01)   # proposals outstanding
        for call in (lambda: b.get_state(), lambda: b.set_state(info, rec, 0)):
            with pytest.raises(MMCError) as e:
                call()
            assert e.value.status == _lib.MMC_ERR_STATE
        b.settle([0, 0])
        assert bits(b.get_state()) == bits(rec)
    with make(a, 1, 9.0) as b:
        b.potential_ewald()
        info, rec = b.state_info(), b.get_state()
        b.volume_trial(20.2, 5.6 / 20.2)                                    # a volume trial is open
        for call in (lambda: b.get_state(), lambda: b.set_state(info, rec, 0)):
            with pytest.raises(MMCError) as e:
                call()
            assert e.value.status == _lib.MMC_ERR_STATE
        b.volume_reject()
        assert bits(b.get_state()) == bits(rec)
