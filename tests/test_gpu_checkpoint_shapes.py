"""Save and resume at the sizes where the two state kernels branch (k_state_pack / k_state_unpack,
mmc_state.hpp), in both of their forms, and the staging around them at every chunk shape.

A workgroup takes a slab of 128 molecules and moves the com and coords sections as double2: an odd
molecule count ends each section in a half-filled word and an 8-byte pad, and a count just past a
multiple of 128 gives a last slab of one molecule.

    N     1 smallest, odd    2 smallest even    3 odd, both pads    127 odd, one ragged slab
        128 exactly one slab    129 a second slab of one molecule    257 three slabs, the last of one

Systems: the first N molecules of a NIST SPC/E configuration in its 20 A box (as
test_gpu_orient.truncated makes them; configuration 1 holds 100 molecules, so 127..129 come from
configuration 2 and 257 from configuration 3, the same box), r_cut 10 A -- homogeneous, the record
form <true> -- and the same prefixes of common.spce_tip3p_mixture, which have no record lines and
take the array form <false> (not at N = 1: one molecule is homogeneous).  Two quaternion systems
(27 and 125 molecules, both odd: the orientation section follows two pads).  R = 5, every replica
with its own coordinates, a few moves after recip_long so that the current S buffer differs
between replicas, temperatures set on every other case.

The reference of a copy kernel is an independent read of the same state: get_replica,
get_orientations, temperatures.  Every comparison is bitwise; there is no tolerance in this file."""
import numpy as np
import pytest

import common
import test_gpu_moves as gm
from metropolismontecarlo_amd import checkpoint
from test_gpu_checkpoint import DPHI, DR, REPLICA0, SEED, T, bits, counts, device_order, make, shifted
from test_gpu_orient import diversify

pytestmark = pytest.mark.gpu

R = 5
TEMPS = 280.0 + 10.0 * np.arange(R)
PRE_STEPS, STEPS = 8, 16
CHUNKS = (1, 2, 5, 7, 0)          # one replica; a ragged last chunk; the request; more than it; the budget's


class Case:
    """One system.  options / kw: how its moves run; forms: the move kernels of the continued chain."""
    quat = False
    rcut = 10.0

    def __init__(self, kind, n, temps):
        self.kind, self.n, self.temps = kind, n, temps
        self.id = f"{kind}-{n}" + ("-temps" if temps else "")
        if kind == "spce":
            self.options = dict(device_moves=1, kernel=2, persistent=0, candidate_lists=1)
            self.kw = dict(n_groups=2, n_threads=2, n_parts=1)
            self.forms = {"wave kernel with lists": dict(kernel=2, persistent=0, candidate_lists=1),
                          "generic kernel": dict(kernel=0)}
        else:                     # (the run options of test_gpu_batch's mixture cases: host proposals, kernel 0)
            self.options = dict(kernel=0)
            self.kw = dict(n_groups=2, n_threads=2, n_parts=3)
            self.forms = {"generic kernel": dict(kernel=0)}

    def arrays(self):
        n = self.n
        k = 1 if n <= 100 else 2 if n <= 200 else 3
        if self.kind == "spce":
            a = common.nist_arrays(k, "unwrapped")
        else:
            a, species = common.spce_tip3p_mixture(k, self.kind)
            assert set(species[:n]) == {0, 1}, "the prefix must hold both species"
        assert a["box"] == 20.0 and a["com"].shape[0] >= n
        return dict(a, com=a["com"][:n], coords=a["coords"][:3 * n], atype=a["atype"][:3 * n], charge=a["charge"][:3 * n])

    def configure(self, b, a):
        """The modes of a batch that is to receive this case's records (set_state configures nothing)."""
        if self.temps:
            b.set_temperatures(TEMPS + 5.0)

    def diversify(self, b, a):
        diversify(b, a, seed=1000 + self.n)              # replicas 1.. : every molecule turned and displaced


class QuatCase(Case):
    """gm.quaternion_system(n, faithful): the replicas start alike and part through their own moves.
    27 molecules at that density are a 9.3 A box, kappa = 0.6: beyond the table kernels (kappa <= 0.5),
    so that system runs on the generic kernel; 125 molecules (15.6 A, kappa = 0.36) run on the wave
    kernel at r_cut 4.5 A, where kappa sqrt(r_cut^2 + 100) = 3.94 is within the erfc table's 4."""
    quat = True

    def __init__(self, n, faithful, rcut, kernel, temps):
        self.kind, self.n, self.temps, self.faithful, self.rcut = "quat", n, temps, faithful, rcut
        self.id = f"quat{1 if faithful else 2}-{n}" + ("-temps" if temps else "")
        self.options = dict(device_moves=1, kernel=kernel, persistent=0)
        self.kw = dict(n_groups=2, n_threads=2, n_parts=1)
        self.forms = {"wave kernel" if kernel == 2 else "generic kernel": dict(kernel=kernel, persistent=0)}

    def arrays(self):
        return gm.quaternion_system(self.n, self.faithful)[0]

    def configure(self, b, a):
        _, quat, db = gm.quaternion_system(self.n, self.faithful)
        b.set_orientations(quat, db, faithful=self.faithful)
        Case.configure(self, b, a)

    def diversify(self, b, a):
        pass


SIZES = (1, 2, 3, 127, 128, 129, 257)
MIX = {2: "interleaved", 3: "minority1", 127: "interleaved", 128: "minority1", 129: "interleaved", 257: "minority1"}
CASES = [Case("spce", n, temps=k % 2 == 1) for k, n in enumerate(SIZES)] \
    + [Case(MIX[n], n, temps=k % 2 == 0) for k, n in enumerate(SIZES) if n in MIX] \
    + [QuatCase(27, True, 4.5, 0, temps=False), QuatCase(125, False, 4.5, 2, temps=True)]


def build(case):
    """(batch, running energies) of the case after its moves; the same every time it is called."""
    a = case.arrays()
    b = make(a, R, case.rcut, case.options)
    try:
        case.configure(b, a)
        if case.temps:
            b.set_temperatures(TEMPS)
        case.diversify(b, a)
        b.recip_long()
        e = b.potential_ewald(as_array=True)["energy"].copy()
        assert np.isfinite(e).all(), e
        n_pre = 60 if case.quat else PRE_STEPS
        e, st = b.run(n_pre, T, DR, DPHI, SEED + 1, energies=e, **case.kw)
        assert st["moves"] == R * n_pre, st
        return b, e
    except BaseException:
        b.close()
        raise


def receiver(case, a, chunk, delivery=-1):
    """A batch of the same system created from shifted coordinates, in the modes of the case."""
    b = make(shifted(a), R, case.rcut, case.options, chunk=chunk)
    try:
        b.set_option("state_delivery", delivery)
        case.configure(b, a)
        b.recip_long()
        return b
    except BaseException:
        b.close()
        raise


@pytest.fixture(scope="module", params=CASES, ids=[c.id for c in CASES])
def src(request):
    """The case's batch after its moves, left alone by every test: its records, info and energies."""
    case = request.param
    b, e = build(case)
    try:
        state = b.get_state()
        assert len(set(bits(row) for row in state)) == R          # every replica has its own state
        yield dict(case=case, b=b, e=e, a=case.arrays(), state=state, info=b.state_info())
    finally:
        b.close()


def replica_reads(b, case):
    """Everything the library reads back of every replica without a state kernel."""
    out = []
    for r in range(R):
        out.extend(b.get_replica(r))
        if case.quat:
            out.append(b.get_orientations(r))
    out.append(b.temperatures())
    return out


def same_reads(x, y, what):
    assert len(x) == len(y)
    for k, (u, v) in enumerate(zip(x, y)):
        assert u.shape == v.shape and bits(u) == bits(v), (what, k)


def sections(info, quat):
    """(offsets, record bytes, the mask of the bytes that belong to a section)."""
    off, rb = checkpoint.record_layout(info)
    n, nk = int(info.n_mol), int(info.nkvecs)
    used = np.zeros(rb, dtype=bool)
    for o, length in ((off[0], 8), (off[1], 8), (off[2], 8), (off[3], 24 * n), (off[4], 72 * n), (off[5], 16 * nk),
                      (off[6], 32 * n if quat else 0)):
        used[o:o + length] = True
    return off, rb, used


# ---- a: records against an independent read ---------------------------------------------------------------
def test_a_record_holds_what_the_batch_reads_back(src):
    case, b, info = src["case"], src["b"], src["info"]
    assert info.n_mol == case.n and info.R == R and info.temps_on == int(case.temps)
    assert info.quat_mode == ((1 if case.faithful else 2) if case.quat else 0)
    for r in range(R):
        rec = checkpoint.split_record(info, src["state"][r])
        com, coords, s_ref = b.get_replica(r)
        assert bits(rec["com"]) == bits(com) and bits(rec["coords"]) == bits(coords), r
        assert rec["box"] == float(src["a"]["box"]) == info.box, r
        assert rec["temperature"] == (TEMPS[r] if case.temps else 0.0), r
        assert rec["flags"] == (2 if case.temps else 0) | (4 if case.quat else 0), r
        assert rec["S"].shape == (info.nkvecs,) and bits(rec["S"]) == bits(device_order(s_ref, info)), r
        assert np.abs(rec["S"]).max() > 0.0
        if case.quat:
            assert bits(rec["quat"]) == bits(b.get_orientations(r)), r
        else:
            assert rec["quat"] is None


# ---- b: every byte outside the sections is zero, in every delivery and chunk shape ---------------------------
def test_b_bytes_outside_the_sections_are_zero_in_every_delivery_and_chunk(src):
    case, b, info, want = src["case"], src["b"], src["info"], src["state"]
    n = case.n
    off, rb, used = sections(info, case.quat)
    pad = 8 * (n % 2)                                    # a change of layout cannot hollow this test out:
    assert off[4] - (off[3] + 24 * n) == pad and off[5] - (off[4] + 72 * n) == pad, off
    assert int((~used).sum()) == 8 + 2 * pad + (rb - off[7]) and want.shape == (R, rb)
    try:
        for delivery in (-1, 0, 1):
            for chunk in CHUNKS:
                b.set_option("state_delivery", delivery)
                b.set_option("state_chunk", chunk)
                got = b.get_state()
                stray = np.argwhere(got[:, ~used])
                assert stray.size == 0, (f"N = {n}, delivery {delivery}, chunk {chunk}: non-zero bytes outside the "
                                         f"sections at (replica, byte) {[(int(r), int(np.flatnonzero(~used)[k])) for r, k in stray[:8]]}")
                assert bits(got) == bits(want), (n, delivery, chunk)
    finally:
        b.set_option("state_delivery", -1)
        b.set_option("state_chunk", 5)


# ---- c: ranges ----------------------------------------------------------------------------------------------
def test_c_ranges_concatenate_to_the_whole(src):
    b, want = src["b"], src["state"]
    try:
        b.set_option("state_chunk", 2)
        # (chunks count from a range's first replica: ranges of one chunk, of less, of two and a ragged third)
        for cuts in ((0, 5), (0, 2, 4, 5), (0, 1, 5), (0, 3, 5), (0, 1, 2, 3, 4, 5), (0, 4, 5)):
            parts = [b.get_state(lo, hi - lo) for lo, hi in zip(cuts, cuts[1:])]
            assert bits(np.concatenate(parts)) == bits(want), cuts
        out = np.zeros((3, want.shape[1]), dtype=np.uint8)
        assert b.get_state(1, 3, out=out) is out and bits(out) == bits(want[1:4])
    finally:
        b.set_option("state_chunk", 5)


# ---- d: round trip into a batch created from shifted coordinates, and the chain after it --------------------
def test_d_a_batch_from_shifted_coordinates_continues_the_chain(src):
    """set_state of all records, then everything read back without a state kernel, then the same
    short call on a source and on the receiver: what only a move kernel reads (the fixed-point
    centres of mass behind the COM scan and the candidate lists, the record lines, the S buffers)
    shows in energies, counts and the records afterwards."""
    case, info, want = src["case"], src["info"], src["state"]
    for form, opts in case.forms.items():
        twin, e = build(case)                            # the chain's source: the fixture's batch is left alone
        dst = None
        try:
            dst = receiver(case, src["a"], chunk=2)      # three chunks, the last ragged, both staging buffers
            assert bits(twin.get_state()) == bits(want) and bits(e) == bits(src["e"]), form
            assert bits(dst.get_state()) != bits(want)
            dst.set_state(info, want)
            assert bits(dst.get_state()) == bits(want), form
            assert checkpoint.info_to_dict(dst.state_info()) == checkpoint.info_to_dict(info)
            same_reads(replica_reads(dst, case), replica_reads(src["b"], case), form)
            assert bits(dst.rdf_sites(50, per_replica=True)) == bits(src["b"].rdf_sites(50, per_replica=True)), form
            out = []
            for b in (twin, dst):
                for k, v in opts.items():
                    b.set_option(k, v)
                listed = b.cand_stats()["list_steps"]
                e1, st = b.run(STEPS, T, DR, DPHI, SEED, energies=e, replica0=REPLICA0, **case.kw)
                cs = b.cand_stats()
                out.append(dict(e=e1, counts=counts(st), state=b.get_state(), reads=replica_reads(b, case),
                                lists=(cs["state"], cs["list_steps"] - listed)))
            x, y = out
            print(f"{case.id}, {form}: counts {x['counts']} / {y['counts']}, lists (state, steps) {x['lists']} / {y['lists']}")
            assert bits(x["e"]) == bits(y["e"]), (case.id, form, x["e"], y["e"])
            assert x["counts"] == y["counts"], (case.id, form)
            differ = [r for r in range(R) if bits(x["state"][r]) != bits(y["state"][r])]
            assert not differ, f"{case.id}, {form}: the records of replicas {differ} differ after {STEPS} steps"
            same_reads(x["reads"], y["reads"], form)
            assert x["counts"][0] == R * STEPS and x["counts"][2] + x["counts"][4] > 0         # moves were accepted
            assert bits(x["state"]) != bits(want)
            if "lists" in form and case.n >= 127:        # the receiver's lists are rebuilt from the unpacked codes
                assert y["lists"][0] == 1 and y["lists"][1] > 0, y["lists"]
        finally:
            twin.close()
            if dst is not None:
                dst.close()


# ---- e: a range written into the middle ---------------------------------------------------------------------
@pytest.mark.parametrize("delivery", (0, 1))
def test_e_a_range_into_the_middle_leaves_the_others(src, delivery):
    case, info, want = src["case"], src["info"], src["state"]
    with receiver(case, src["a"], chunk=2 if delivery == 0 else 0, delivery=delivery) as dst:
        e = dst.potential_ewald(as_array=True)["energy"].copy()
        dst.run(PRE_STEPS, T, DR, DPHI, SEED + 2, energies=e, **case.kw)            # (S buffers of both parities)
        before, reads = dst.get_state(), replica_reads(dst, case)
        rec = np.ascontiguousarray(want[1:4])
        assert bits(before[1:4]) != bits(rec)
        dst.set_state(info, rec, r0=1)
        after, now = dst.get_state(), replica_reads(dst, case)
        assert bits(after[1:4]) == bits(rec)
        assert bits(after[0]) == bits(before[0]) and bits(after[4]) == bits(before[4])
        per = len(reads) // R                                                        # arrays per replica (then temperatures)
        ours = replica_reads(src["b"], case)
        for r in range(R):
            same_reads(now[per * r:per * (r + 1)], (ours if 1 <= r < 4 else reads)[per * r:per * (r + 1)], r)
        if case.temps:
            assert bits(now[-1]) == bits(np.concatenate([TEMPS[:1] + 5.0, TEMPS[1:4], TEMPS[4:] + 5.0]))
        else:
            assert not now[-1].any()
