"""mmc_batch_solute_forces (include/mmc_hip.h, "A fixed solute: the mean force, field and potential on
it") on the GPU: every output of every replica against the numpy restatement solute_force_ref.replica on the
replica's own get_replica data, within 1e-12 A + 1e-300 (A: the same sum over the absolute values of its
terms), which tests/test_solute_force_host.py pins on the oracle by central differences.  Then what the
launch must not change, bit for bit, the flags, and the refusals.  Every comparison prints the largest
|x - ref| / A it met."""
import ctypes as C

import numpy as np
import pytest

import common
import forces_ref as fr
import solute_chain_ref as scr
import solute_force_ref as ref
import solute_ref as sr
from metropolismontecarlo_amd import _lib
from metropolismontecarlo_amd import structs

pytestmark = pytest.mark.gpu

LJ, QQ, T = 8.5, 9.5, sr.T
NAMES = ("cation", "dipole", "methane", "synthetic5", "synthetic16")


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def cfg3():
    return common.nist_arrays(3, "unwrapped")     # 300 SPC/E in 20 A


def solute_of(name, a):
    return {"methane": sr.methane, "cation": sr.cation, "dipole": sr.dipole, "mea": lambda a: sr.mea(),
            "synthetic5": lambda a: sr.synthetic(a, 5, seed=3),
            "synthetic16": lambda a: sr.synthetic(a, 16, seed=7)}[name](a)


def make_batch(a, reps, lj=LJ, qq=QQ, alpha=5.6):
    """A batch of len(reps) replicas of system `a`, replica r at reps[r] = (com, coords)."""
    from metropolismontecarlo_amd.device import Batch
    b = Batch(len(reps), a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
              alpha / a["box"], structs.factor, lj, qq)
    for r, (com, coords) in enumerate(reps):
        b.set_replica(r, com, coords)
    b.recip_long()
    return b


def shifted(a, R):
    """R configurations of their own: `a` translated rigidly by a vector per replica and wrapped by COM."""
    return [fr.shifted_replica(a, k) for k in range(R)]


def corner(box):
    return np.array([box - 0.4, 0.3, box - 0.2])


def face(box):
    return np.array([box - 0.3, 0.45 * box, 0.6 * box])


def with_solute(b, sol, mol):
    b.set_solute(sol, mol)
    b.recip_long()
    return b


def compare(su, sol, mol, b, out, what, S_of=None):
    """Every replica of `out` against the restatement; returns (the restatements, flags seen)."""
    refs, worst = [], 0.0
    for r in range(b.R):
        rr, w = ref.check(su, sol, mol, b, r, out, what, S=None if S_of is None else S_of(r))
        refs.append(rr)
        worst = max(worst, w)
    flags = [rr["flags"] for rr in refs]
    print(f"{what}: worst |x - ref| / A = {worst:.3g}, flagged {sum(1 for f in flags if f)} of {b.R}")
    return refs, flags


# ---- shapes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", (1, 3, 70))
@pytest.mark.parametrize("N", (1, 2, 65, 257))
def test_every_output_against_the_restatement(orc, cfg3, N, R):
    """A lane with 0, 1, 2 and 5 waters; one, three and seventy replicas, each from a configuration of its
    own; the solutes take turns over the shapes, at the corner of the box."""
    name = NAMES[(3 * (1, 2, 65, 257).index(N) + (1, 3, 70).index(R)) % len(NAMES)]
    a = sr.first_molecules(cfg3, N)
    sol, box = solute_of(name, a), float(a["box"])
    mol = sr.placed(sol.offsets, corner(box), sr.rotation(np.random.default_rng(N + R)))
    su = ref.setup(a, orc, box, LJ, QQ)
    with make_batch(a, shifted(a, R)) as b:
        with_solute(b, sol, mol)
        out = b.solute_forces(details=True)
        refs, flags = compare(su, sol, mol, b, out, f"{name} N={N} R={R}")
    assert sum(1 for f in flags if f == 0) >= (R + 1) // 2        # most replicas are unflagged
    if N >= 65:
        assert all(rr["n_counted"] > 0 for rr in refs)


@pytest.mark.parametrize("name", NAMES)
def test_every_solute_at_257_and_a_face(orc, cfg3, name):
    a = sr.first_molecules(cfg3, 257)
    sol, box = solute_of(name, a), float(a["box"])
    su = ref.setup(a, orc, box, LJ, QQ)
    with make_batch(a, shifted(a, 3)) as b:
        for where, c in (("face", face(box)), ("corner", corner(box))):
            mol = sr.placed(sol.offsets, c, sr.rotation(np.random.default_rng(5)))
            with_solute(b, sol, mol)
            refs, flags = compare(su, sol, mol, b, b.solute_forces(details=True), f"{name} at the {where}")
            assert any(f == 0 for f in flags) and all(rr["n_counted"] > 0 for rr in refs)


def test_the_decks_mea(orc):
    """The 11-site monoethanolamine of the decks in 65 waters of its TIP3P lattice."""
    a = sr.first_molecules(sr.tip3p_lattice(), 65)
    sol, box = sr.mea(), float(a["box"])
    su = ref.setup(a, orc, box, sr.MEA_RCUT, sr.MEA_RCUT, sr.MEA_ALPHA)
    mol = sr.placed(sol.offsets, corner(box), sr.rotation(np.random.default_rng(9)))
    with make_batch(a, shifted(a, 3), sr.MEA_RCUT, sr.MEA_RCUT, sr.MEA_ALPHA) as b:
        with_solute(b, sol, mol)
        compare(su, sol, mol, b, b.solute_forces(details=True), "mea")


# ---- gates --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("dipole", "methane"))
def test_both_gates_from_either_side(orc, cfg3, name):
    """solute_ref.gate_cases: the reference point 1e-12 (relative) either side of both COM gates of two
    waters, along three directions, at cutoffs (10, 8).  The qq gate holds for the uncharged solute too."""
    a = sr.first_molecules(cfg3, 257)
    sol, box = solute_of(name, a), float(a["box"])
    lj, qq = 10.0, 8.0
    su = ref.setup(a, orc, box, lj, qq)
    com = np.asarray(a["com"])
    mols, tags = sr.gate_cases(com, box, sol, lj, qq)
    sides, worst = {}, 0.0
    with make_batch(a, [(a["com"], a["coords"])], lj, qq) as b:
        for mol, (j, gi, di, inside) in zip(mols, tags):
            with_solute(b, sol, mol)
            rr, w = ref.check(su, sol, mol, b, 0, b.solute_forces(details=True), f"gate {j, gi, di, inside}")
            worst = max(worst, w)
            c2 = (fr.vector1D(com[j], mol[-1], box) ** 2)
            c2 = (c2[0] + c2[1]) + c2[2]
            # (the LJ gate of 10 A is half the box: a COM beyond it takes its image and lands inside again,
            # in vector1D's arithmetic, which the kernel and the restatement share)
            assert gi == 0 or (c2 < qq ** 2) == inside
            sides[(j, gi, di, inside)] = rr
    # the gate decides something: across it the LJ force (gate 0) or the real-space part (gate 1) changes
    changed = [0, 0]
    for (j, gi, di, inside), rr in sides.items():
        if inside:
            other = sides[(j, gi, di, False)]
            key = "site_lj" if gi == 0 else "real"
            changed[gi] += bool(np.abs(rr[key] - other[key]).max() > 1e-9 * np.abs(rr[key]).max())
    print(f"gates {name}: worst |x - ref| / A = {worst:.3g}, pairs of placements the gate tells apart (lj, qq) {changed}")
    assert changed[1] == 6 and changed[0] >= 1


# ---- the committed S(k) -------------------------------------------------------------------------------
def test_after_a_chain_of_accepted_moves_and_with_the_oracles_s_of_k(orc, cfg3):
    """S(k) as the moves update it incrementally: against the restatement with the replica's own S(k), and
    with the oracle's RecipLong of the same N + 1 coordinates; recip_out alone gives the same bits."""
    a = sr.first_molecules(cfg3, 257)
    sol, box = sr.synthetic(a, 5, seed=3), float(a["box"])
    mol = sr.placed(sol.offsets, corner(box), sr.rotation(np.random.default_rng(2)))
    su = ref.setup(a, orc, box, LJ, QQ)
    so = sr.SoluteOracle(orc, a, sol, LJ, QQ)
    with make_batch(a, shifted(a, 3)) as b:
        with_solute(b, sol, mol)
        S0 = [b.get_replica(r)[2].copy() for r in range(3)]
        b.set_option("device_moves", 1)
        b.run(400, T, 0.3, 0.2, seed=21)
        assert all(np.any(b.get_replica(r)[2] != S0[r]) for r in range(3))       # moves were accepted
        out = b.solute_forces(details=True)
        compare(su, sol, mol, b, out, "after 400 steps, own S(k)")

        def oracle_S(r):
            com, coords, _ = b.get_replica(r)
            return scr.N1(so, com, coords, mol, box).ew.sumQExpOld
        compare(su, sol, mol, b, out, "after 400 steps, the oracle's S(k)", S_of=oracle_S)
        alone = np.full_like(out["recip"], 7.0)
        _lib.check(b._L.mmc_batch_solute_forces(b._h, None, None, None, None, None, alone.ctypes.data_as(_lib._dp), None))
        assert alone.tobytes() == out["recip"].tobytes()


def test_an_uncharged_solute_has_field_and_phi_and_does_not_stale_s_of_k(orc, cfg3):
    a = sr.first_molecules(cfg3, 257)
    sol, box = sr.methane(a), float(a["box"])
    mol = sr.placed(sol.offsets, face(box))
    su = ref.setup(a, orc, box, LJ, QQ)
    with make_batch(a, shifted(a, 3)) as b:
        b.set_solute(sol, mol)                       # (no recip_long: S(k) is not stale)
        assert not b.state_info().s_stale
        out = b.solute_forces(details=True)
        refs, flags = compare(su, sol, mol, b, out, "methane, S(k) untouched")
    assert any(f == 0 for f in flags)
    ok = [r for r in range(3) if flags[r] == 0]
    assert all(np.abs(out["phi"][r]).min() > 0 and np.abs(out["field"][r]).max() > 0 for r in ok)
    assert all(np.array_equal(out["force"][r], out["site_lj"][r, 0]) for r in ok)      # q = 0: the force is site_lj


# ---- launch independence ------------------------------------------------------------------------------
def test_no_launch_shard_or_set_of_outputs_changes_a_bit(cfg3):
    a = sr.first_molecules(cfg3, 65)
    sol, box = sr.synthetic(a, 16, seed=7), float(a["box"])
    mol = sr.placed(sol.offsets, corner(box), sr.rotation(np.random.default_rng(4)))
    reps = shifted(a, 70)
    names = ("force", "torque", "site_lj", "field", "phi", "recip", "flags")
    with make_batch(a, reps) as b:
        with_solute(b, sol, mol)
        full = b.solute_forces(details=True)
        again = b.solute_forces(details=True)                                        # a second call
        b.set_option("wave_wgs", 1)                                                  # one workgroup walks all 70
        one = b.solute_forces(details=True)
        b.set_option("wave_wgs", 0)
        for k in names:
            assert full[k].tobytes() == again[k].tobytes() == one[k].tobytes(), k
        assert np.any(full["flags"] == 0) and np.any(full["force"] != 0.0)
        plain = b.solute_forces()
        assert list(plain) == ["force", "torque", "flags"] and all(plain[k].tobytes() == full[k].tobytes() for k in plain)
        for k in names:                                                              # each output alone
            alone = np.full_like(full[k], 3)
            ptrs = [alone.ctypes.data_as(C.POINTER(C.c_uint8 if k == "flags" else C.c_double)) if n == k else None
                    for n in names]
            _lib.check(b._L.mmc_batch_solute_forces(b._h, *ptrs))
            assert alone.tobytes() == full[k].tobytes(), k
    # shards of three replicas, replica0 = 3 k (not of one: RecipLong of a one-replica batch is another
    # kernel, k_potential_one, whose S(k) differs from the batch kernels' in the last bits)
    for r0 in (0, 33, 66):
        with make_batch(a, reps[r0:r0 + 3]) as s:
            with_solute(s, sol, mol)
            part = s.solute_forces(details=True)
        for k in names:
            assert part[k].tobytes() == full[k][r0:r0 + 3].tobytes(), (r0, k)


# ---- flags --------------------------------------------------------------------------------------------
def test_a_planted_overlap_and_an_atom_on_a_site(orc, cfg3):
    a = sr.first_molecules(cfg3, 257)
    sol, box = sr.cation(a), float(a["box"])
    su = ref.setup(a, orc, box, LJ, QQ)
    reps = [(com.copy(), coords.copy()) for com, coords in shifted(a, 4)]
    # the site r^2 = 0.3 from the O of water 40 of replica 1, and exactly on its first H in replica 2
    mol = sr.placed(sol.offsets, reps[1][1][120] + np.array([0.5, 0.2, 0.1]))
    t = mol[0] - reps[2][1][121]
    reps[2][0][40] += t
    reps[2][1][120:123] += t
    with make_batch(a, reps) as b:
        with_solute(b, sol, mol)
        out = b.solute_forces(details=True)
        refs, flags = compare(su, sol, mol, b, out, "planted")
    assert flags[1] == 1 and flags[2] & 2 and out["flags"][1] == 1 and out["flags"][2] & 2
    assert flags[0] == 0 and np.any(out["force"][0] != 0) and np.any(out["phi"][0] != 0)   # the neighbours are unaffected
    for k in ("force", "torque", "site_lj", "field", "phi", "recip"):
        assert not np.any(out[k][1]) and not np.any(out[k][2]), k


# ---- read-only, refusals ------------------------------------------------------------------------------
def test_calls_between_the_runs_of_a_chain_change_nothing(cfg3):
    a = sr.first_molecules(cfg3, 65)
    sol, box = sr.dipole(a), float(a["box"])
    mol = sr.placed(sol.offsets, corner(box))
    states = []
    for interleave in (False, True):
        with make_batch(a, shifted(a, 3)) as b:
            with_solute(b, sol, mol)
            b.set_option("device_moves", 1)
            e = b.potential_ewald(as_array=True)["energy"].copy()
            for leg in range(3):
                if interleave:
                    b.solute_forces(details=True)
                b.run(60, T, 0.3, 0.2, seed=8, energies=e)
            if interleave:
                b.solute_forces()
            states.append((e.tobytes(), [tuple(x.tobytes() for x in b.get_replica(r)) for r in range(3)]))
    assert states[0] == states[1]


def test_refusals_leave_the_outputs_untouched(cfg3):
    a = sr.first_molecules(cfg3, 65)
    sol, box = sr.cation(a), float(a["box"])
    mol = sr.placed(sol.offsets, face(box))

    def refused(b, word):
        mine = {"force": np.full((b.R, 3), 5.0), "torque": np.full((b.R, 3), 5.0), "flags": np.full(b.R, 9, dtype=np.uint8)}
        with pytest.raises(_lib.MMCError, match="MMC_ERR_STATE.*" + word):
            b.solute_forces(out=mine)
        assert all(np.all(v == (9 if k == "flags" else 5.0)) for k, v in mine.items())
    with make_batch(a, shifted(a, 2)) as b:
        refused(b, "no solute")
        b.set_solute(sol, mol)
        refused(b, "stale")                                      # a charged solute before recip_long
        b.recip_long()
        b.solute_forces()
        com, coords, _ = b.get_replica(0)
        b.eval([1, 1], [com[0], com[0]], [coords[:3], coords[:3]])
        refused(b, "outstanding")
        b.settle(np.zeros(2, dtype=np.int32))
        b.solute_forces()
        b.set_solute(None)
        refused(b, "no solute")
