"""A restatement of the reference's Loop() (Ewald/main.jl:487-644) for the tests, with the oracle
stepping the same chain in lockstep.

The driver sweeps molecules, draws translations and rotations with moves.py's formulas
(auxillary.jl:94-114, quaternions.jl:158-182, main.jl:519-552), decides with Metropolis(delta / T)
on a seeded host RNG (auxillary.jl:104-114) and keeps the caller's arrays as Loop() keeps them:
accept -> sumQExpOld = copy(sumQExpNew) (:621), reject -> the molecule and sumQExpNew restored
(:623-628), Adjust! / Adjust_rot! between blocks of moves (adjust.jl).  It runs over one of two
call forms:

* ReferenceForm -- the five reference calls per move (LJ_poly_dU + EwaldShort before and after the
  move, RecipMove when there is no overlap: main.jl:491-506,557-582), or for coulombStyle "bare"
  LJ_poly_dU(i, system) + CoulombReal(qq_r, qq_q, box, i, system) (:494-499,560-565) and no
  RecipMove.  `surface` is metropolismontecarlo_amd.api on the GPU, or OracleSurface (the same
  signatures served by the CPU oracle) on the CPU.
* TrialForm -- one device.Context.trial_move + accept_move / reject_move per move.

Lockstep holds its own oracle System and Ewald, applies the decisions the driver took, and checks
every call: LJ energy and virial, real-space energy and virial, the overlap flag, RecipMove's dU,
the caller's sumQExpOld after an accepted move.  A decision whose margin |exp(-x) - u| is below
1e-9 is logged, not asserted: Lockstep.close_calls, named in every failure message of the
lockstep and in a warning at the end of the run.

Two departures from the letter of Loop(), each for a reason the reference states itself:
* rotations use the orthogonal rotation matrix (moves.q_to_a(faithful=False)): the reference's
  element (2,3) typo (quirk Q12) would deform every rotated molecule;
* qq_r, the coordinates the "bare" style's CoulombReal reads, is soa.coords itself: Loop()'s
  `qq_r[...] = ra_new` (main.jl:554) is commented out, which leaves CoulombReal on the starting
  configuration.
"""
import math
import warnings

import numpy as np

from metropolismontecarlo_amd import moves as mv
from metropolismontecarlo_amd import structs
from metropolismontecarlo_amd.structs import Moves, Properties, Properties2, Requirements, Tables

RCUT = 10.0
T = 298.15
MARGIN = 1e-9


def near(x, ref, scale=1.0, tol=1e-9):
    """|x - ref| within tol of the larger of |ref| and `scale` (the magnitude of the terms a
    difference was formed from)."""
    return abs(x - ref) <= tol * max(abs(ref), scale, 1.0)


# ---- the chain's state as the caller holds it -----------------------------------------------------
class LoopState:
    """moa / soa / vdwTable / ewald / totProps of main.jl:242-303, the body-fixed sites db and
    quaternions of every molecule (a molecule starts at the identity, its sites as they are), the
    step-size controllers and the host RNG."""

    def __init__(self, a, ewald, seed, dr_max=0.3166, dphi_max=0.05):
        self.a = a
        self.box = float(a["box"])
        self.moa = structs.make_moa(np.array(a["com"], dtype=float).reshape(-1, 3),
                                    a["first_atom"], a["last_atom"])
        self.soa = structs.make_soa(np.array(a["coords"], dtype=float).reshape(-1, 3), a["atype"],
                                    a["charge"])
        self.vdwTable = _table(a)
        self.ewald = ewald
        self.totProps = Properties2(T, 0.0331, 0.0, dr_max, dphi_max, 0.3, 0, 0, [], RCUT, RCUT,
                                    self.box)
        n = self.n_mol
        self.quat = np.tile([1.0, 0.0, 0.0, 0.0], (n, 1))
        self.db = [self.atoms(i) - self.moa.COM[i - 1] for i in range(1, n + 1)]
        self.trans, self.rot = Moves(), Moves()
        self.rng = np.random.default_rng(seed)
        # the legacy argument bundle of the "bare" style's calls, on the same arrays
        tma = np.stack([self.moa.firstAtom, self.moa.lastAtom], axis=1)
        self.system = Requirements(self.moa.COM, self.soa.coords, n, len(self.soa.coords),
                                   len(self.soa.coords), tma, [], [], [], self.soa.atype,
                                   self.vdwTable, self.box, RCUT)

    @property
    def n_mol(self):
        return len(self.moa.firstAtom)

    def span(self, i):
        return self.moa.firstAtom[i - 1] - 1, self.moa.lastAtom[i - 1]

    def atoms(self, i):
        f, l = self.span(i)
        return self.soa.coords[f:l].copy()

    def place(self, i, com, atoms):
        f, l = self.span(i)
        self.moa.COM[i - 1] = com
        self.soa.coords[f:l] = atoms

    def propose(self, i):
        """main.jl:516-550: (kind, COM, atoms, quaternion) of a translation or a rotation."""
        p = self.totProps
        if self.rng.random() < 0.5:                                       # :519
            self.trans.attempt += 1
            rnew = mv.random_translate_vector(p.dr_max, self.moa.COM[i - 1], self.box, self.rng)
            ei = self.quat[i - 1]
            kind = "trans"
        else:
            self.rot.attempt += 1
            rnew = self.moa.COM[i - 1].copy()
            ei = mv.random_rotate_quaternion(p.dphi_max, self.quat[i - 1], self.rng)
            kind = "rot"
        ra_new = mv.space_fixed_atoms(rnew, ei, self.db[i - 1], faithful=False)   # :543-549
        return kind, np.asarray(rnew, dtype=float), ra_new, ei

    def adjust(self):
        """main.jl:632-638 (Adjust!, Adjust_rot!); a controller without attempts since its last
        call is left alone (adjust.jl would divide by zero)."""
        for moves, attr in ((self.trans, "dr_max"), (self.rot, "dphi_max")):
            if moves.attempp and moves.attempt == moves.attempp:
                continue
            moves.d_max = getattr(self.totProps, attr)
            mv.Adjust(moves, self.box)
            setattr(self.totProps, attr, moves.d_max)


def _table(a):
    t = Tables.__new__(Tables)
    t.eps_ij = np.array(a["eps"], dtype=float)
    t.sig_ij = np.array(a["sig"], dtype=float)
    return t


# ---- the reference's calls served by the CPU oracle ----------------------------------------------
class OracleSurface:
    """The api.py signatures Loop() uses, answered by oracle/mmc_oracle.c on the caller's arrays
    as they are at the call: the stand-in of the HIP library for the CPU test of the driver."""

    def __init__(self, a):
        from oracle import oracle as orc
        self.orc = orc
        self.a = a

    def _sys(self, moa, soa, box):
        s = self.orc.System(moa.COM, moa.firstAtom, moa.lastAtom, soa.coords, self.a["atype"],
                            self.a["charge"], self.a["eps"], self.a["sig"], box)
        return s

    def PrepareEwaldVariables(self, box):
        return self.orc.Ewald(5.6 / box, 5, 27, box, factor=structs.factor)

    def LJ_poly_ΔU(self, i, *args):
        if len(args) == 1:
            system = args[0]
            s = self.orc.System(system.rm, system.thisMol_theseAtoms[:, 0],
                                system.thisMol_theseAtoms[:, 1], system.ra, system.atomTypes,
                                self.a["charge"], self.a["eps"], self.a["sig"], system.box)
            return self.orc.lj_poly_du(i, s, system.r_cut)
        moa, soa, _, r_cut, box = args
        return self.orc.lj_poly_du(i, self._sys(moa, soa, box), r_cut)

    def EwaldShort(self, i, moa, soa, sim_props, ewald, box):
        return self.orc.ewald_short(i, self._sys(moa, soa, box), ewald, sim_props.qq_rcut)

    def CoulombReal(self, qq_r, qq_q, box, i, system):
        s = self.orc.System(system.rm, system.thisMol_theseAtoms[:, 0],
                            system.thisMol_theseAtoms[:, 1], qq_r, system.atomTypes, qq_q,
                            self.a["eps"], self.a["sig"], box)
        return self.orc.coulomb_real(i, s, system.r_cut)

    def RecipMove(self, box, ewald, r_old, r_new, qq_q):
        ewald.sumQExpNew = np.ascontiguousarray(ewald.sumQExpNew, dtype=np.complex128)
        return self.orc.recip_move(box, ewald, r_old, r_new, qq_q), ewald

    def potential(self, moa, soa, tot, ewald, vdwTable, sim_props, coulomb_style=None):
        s = self._sys(moa, soa, sim_props.box)
        ewald.sumQExpOld = np.zeros(ewald.NKVECS, dtype=np.complex128)
        ewald.sumQExpNew = np.zeros(ewald.NKVECS, dtype=np.complex128)
        if coulomb_style is None:
            t = self.orc.potential_wolf(s, ewald, sim_props.LJ_rcut, sim_props.qq_rcut,
                                        literal_prefactor=False)
        else:
            t = self.orc.potential_ewald(s, ewald, sim_props.LJ_rcut, sim_props.qq_rcut)
        tot = Properties() if tot is None else tot
        tot.energy += t["energy"]
        tot.virial += t["virial"]
        tot.coulomb += t["coulomb"]
        return tot


def bare_total(orc, s, factor, r_cut=RCUT):
    """The energy whose changes the "bare" style's moves add up (main.jl:491-499,557-565): the LJ
    sum of potential() plus factor / 2 sum_i CoulombReal(i)."""
    lj = sum(orc.lj_poly_du(i, s, r_cut)[0] for i in range(1, s.n_mol + 1)) / 2
    qq = sum(orc.coulomb_real(i, s, r_cut)[0] for i in range(1, s.n_mol + 1))
    return lj + qq * factor / 2


# ---- the oracle's own copy of the chain -------------------------------------------------------------
class Lockstep:
    """The oracle stepping the driver's chain on a System / Ewald of its own."""

    def __init__(self, a, style="ewald"):
        from oracle import oracle as orc
        self.orc = orc
        self.a = a
        self.style = style
        self.s = orc.System(a["com"], a["first_atom"], a["last_atom"], a["coords"], a["atype"],
                            a["charge"], a["eps"], a["sig"], a["box"])
        self.ew = orc.Ewald(5.6 / self.s.box, 5, 27, self.s.box, factor=structs.factor)
        self.close_calls = []
        self.checked = 0
        self.start_total = self.total()      # fills ew.sumQExpOld / New (RecipLong, energy.jl:1008)

    def total(self):
        if self.style == "bare":
            return bare_total(self.orc, self.s, self.ew.factor)
        return self.orc.potential_ewald(self.s, self.ew, RCUT, RCUT)["energy"]

    def span(self, i):
        return self.s.first_atom[i - 1] - 1, self.s.last_atom[i - 1]

    def _terms(self, i):
        lj = self.orc.lj_poly_du(i, self.s, RCUT)
        if self.style == "bare":
            e, ov = self.orc.coulomb_real(i, self.s, RCUT)
            return lj, (e * self.ew.factor, 0.0, ov)
        return lj, self.orc.ewald_short(i, self.s, self.ew, RCUT)

    def move(self, i, com_new, atoms_new):
        """The calls of one move (main.jl:491-582) on the oracle's chain; leaves the chain in its
        old state and ew.sumQExpNew as RecipMove leaves it."""
        f, l = self.span(i)
        rm_old, ra_old = self.s.com[i - 1].copy(), self.s.coords[f:l].copy()
        lj_old, q_old = self._terms(i)
        self.s.com[i - 1], self.s.coords[f:l] = com_new, atoms_new
        lj_new, q_new = self._terms(i)
        self.s.com[i - 1], self.s.coords[f:l] = rm_old, ra_old
        overlap = q_old[2] or q_new[2]
        recip = 0.0
        if not overlap and self.style != "bare":
            recip = self.orc.recip_move(self.s.box, self.ew, ra_old, np.asarray(atoms_new, float),
                                        self.s.charge[f:l])
        self.pending = (i, np.array(com_new, dtype=float), np.array(atoms_new, dtype=float))
        delta = (lj_new[0] + q_new[0]) - (lj_old[0] + q_old[0]) + recip
        return dict(lj_old=lj_old, q_old=q_old, lj_new=lj_new, q_new=q_new, recip=recip,
                    overlap=bool(overlap), delta=delta,
                    d=np.array([lj_new[0] - lj_old[0], q_new[0] - q_old[0], recip,
                                (lj_new[1] + q_new[1]) - (lj_old[1] + q_old[1]) + recip / 3]))

    def note_decision(self, delta, u, what):
        """Loop()'s decision is the device's; record the ones the oracle's delta could flip."""
        if u is not None and abs(math.exp(-delta / T) - u) < MARGIN:
            self.close_calls.append((what, delta, u))

    def report(self):
        """The close calls so far, for a failure message."""
        if not self.close_calls:
            return ""
        return f" [decisions within {MARGIN} of flipping: {self.close_calls}]"

    def settle(self, accepted):
        i, com, atoms = self.pending
        if accepted:
            f, l = self.span(i)
            self.s.com[i - 1], self.s.coords[f:l] = com, atoms
            self.ew.sumQExpOld = self.ew.sumQExpNew.copy()               # main.jl:621
        else:
            self.ew.sumQExpNew = self.ew.sumQExpOld.copy()               # :628

    def check_calls(self, got, ref, what):
        """Per-call comparison of a ReferenceForm move with the oracle's."""
        bad = []
        for k in ("lj_old", "lj_new"):
            if not (near(got[k][0], ref[k][0]) and near(got[k][1], ref[k][1], abs(ref[k][0]))):
                bad.append((k, got[k], ref[k]))
        for k in ("q_old", "q_new"):
            if got[k][2] != ref[k][2] or not (near(got[k][0], ref[k][0])
                                              and near(got[k][1], ref[k][1], abs(ref[k][0]))):
                bad.append((k, got[k], ref[k]))
        if got["overlap"] != ref["overlap"] or abs(got["recip"] - ref["recip"]) > 1e-7:
            bad.append(("recip", got["recip"], ref["recip"], got["overlap"], ref["overlap"]))
        assert not bad, f"{what}: {bad}{self.report()}"
        self.checked += 1

    def check_d(self, d, overlap, ref, what):
        """A TrialForm move's d[4] against the oracle's: each a difference of terms, compared at
        1e-9 of those terms' size (RecipMove's at 1e-7 K)."""
        lj_scale = abs(ref["lj_old"][0]) + abs(ref["lj_new"][0])
        q_scale = abs(ref["q_old"][0]) + abs(ref["q_new"][0])
        v_scale = abs(ref["lj_old"][1]) + abs(ref["lj_new"][1]) + q_scale
        ok = (overlap == ref["overlap"] and near(d[0], ref["d"][0], lj_scale)
              and near(d[1], ref["d"][1], q_scale) and abs(d[2] - ref["d"][2]) <= 1e-7
              and near(d[3], ref["d"][3], v_scale))
        assert ok, (f"{what}: d={list(d)} oracle={list(ref['d'])} overlap {overlap}/{ref['overlap']}"
                    f"{self.report()}")
        self.checked += 1

    def check_s_old(self, s_old, what):
        scale = np.abs(self.ew.sumQExpOld).max()
        err = np.abs(np.asarray(s_old) - self.ew.sumQExpOld).max()
        assert err < 1e-11 * scale, (f"{what}: caller's sumQExpOld off the oracle's by {err}"
                                     f"{self.report()}")


# ---- the two call forms ----------------------------------------------------------------------------
class ReferenceForm:
    """The body of Loop() over the reference's calls (main.jl:491-629) on st's arrays.
    commit: "copy" (main.jl:621,628) or "api" (RecipCommit / RecipRollback)."""

    def __init__(self, surface, st, style="ewald", commit="copy"):
        self.f, self.st, self.style, self.commit = surface, st, style, commit

    def _terms(self, i):
        st, f = self.st, self.f
        if self.style == "bare":
            e, v = f.LJ_poly_ΔU(i, st.system)                                          # (:491)
            q, ov = f.CoulombReal(st.soa.coords, st.soa.charge, st.box, i, st.system)  # :495-496
            return (e, v), (q * st.ewald.factor, 0.0, ov)                               # :497-498
        e, v = f.LJ_poly_ΔU(i, st.moa, st.soa, st.vdwTable, RCUT, st.box)             # :491
        return (e, v), f.EwaldShort(i, st.moa, st.soa, st.totProps, st.ewald, st.box)  # :501-502

    def move(self, i, com_new, atoms_new):
        st = self.st
        lj_old, q_old = self._terms(i)
        self.rm_old, self.ra_old = st.moa.COM[i - 1].copy(), st.atoms(i)              # :514-515
        self.i = i
        st.place(i, com_new, atoms_new)                                                 # :527,552
        ra_new = st.atoms(i)
        lj_new, q_new = self._terms(i)                                                  # :557-571
        overlap = bool(q_old[2] or q_new[2])                                            # :574-578
        recip = 0.0
        if not overlap and self.style != "bare":                                        # :580
            f, l = st.span(i)
            recip, st.ewald = self.f.RecipMove(st.box, st.ewald, self.ra_old, ra_new,
                                               st.soa.charge[f:l])                      # :581-587
        delta = (lj_new[0] + q_new[0]) - (lj_old[0] + q_old[0]) + recip                 # :593
        dvir = (lj_new[1] + q_new[1]) - (lj_old[1] + q_old[1]) + recip / 3              # :602
        return dict(lj_old=lj_old, q_old=q_old, lj_new=lj_new, q_new=q_new, recip=recip,
                    overlap=overlap, delta=delta, dvir=dvir)

    def settle(self, accepted):
        st = self.st
        if accepted:
            if self.commit == "api":
                from metropolismontecarlo_amd.api import RecipCommit
                RecipCommit(st.ewald)
            else:
                st.ewald.sumQExpOld = np.array([item for item in st.ewald.sumQExpNew])  # :621
        else:
            st.place(self.i, self.rm_old, self.ra_old)                                  # :623-624
            if self.commit == "api":
                from metropolismontecarlo_amd.api import RecipRollback
                RecipRollback(st.ewald)
            else:
                st.ewald.sumQExpNew = np.array([item for item in st.ewald.sumQExpOld])  # :628

    def s_old(self):
        return None if self.style == "bare" else self.st.ewald.sumQExpOld


class TrialForm:
    """One mmc_trial_move per move (device.Context.trial_move) and its accept / reject; st's
    arrays follow the accepted moves."""

    def __init__(self, ctx, st):
        self.ctx, self.st = ctx, st

    def move(self, i, com_new, atoms_new):
        d, ov = self.ctx.trial_move(i, com_new, atoms_new, RCUT, RCUT)
        self.pending = (i, com_new, atoms_new)
        return dict(d=d, overlap=ov, delta=d[0] + d[1] + d[2], dvir=d[3])

    def settle(self, accepted):
        if accepted:
            self.ctx.accept_move()
            self.st.place(*self.pending)
        else:
            self.ctx.reject_move()

    def s_old(self):
        return None


# ---- the loop ----------------------------------------------------------------------------------------
def order_of(kind, n_mol, n_moves, rng):
    """The molecules of n_moves moves: "sweep" (main.jl:490, wrapping n_mol -> 1), "random", or
    "twice" (each molecule of the sweep twice in a row), or a list of molecules swept in its
    order (a system whose other molecules Loop() cannot move: RecipMove's n == 3)."""
    if not isinstance(kind, str):
        return [int(kind[k % len(kind)]) for k in range(n_moves)]
    if kind == "sweep":
        return [1 + k % n_mol for k in range(n_moves)]
    if kind == "random":
        return [int(x) for x in rng.integers(1, n_mol + 1, size=n_moves)]
    if kind == "twice":
        return [1 + (k // 2) % n_mol for k in range(n_moves)]
    raise ValueError(kind)


def run(form, st, order, n_moves, lockstep=None, total=None, adjust_every=50, script=None,
        between=None, check_total=None, block=None):
    """n_moves iterations of Loop()'s body.  Returns (running energy, records).

    script: {move index: dict(mol=, com=, atoms=, accept=)} -- a scripted move replaces the drawn
      one (the RNG still draws, so the rest of the run stays the same; the replaced draw is not
      counted as an attempt for Adjust!), `accept` forces the decision (True / False; None:
      Metropolis).  dict(accept=) alone forces the decision of the drawn move, which stays a
      translation or rotation for Adjust!.
    between: {move index: callable(st, running) -> running} run before that move.
    check_total(st, running, k): called after every `block` moves and at the end."""
    script = {} if script is None else script
    between = {} if between is None else between
    mols = order_of(order, st.n_mol, n_moves, np.random.default_rng(st.rng.integers(1 << 62)))
    running = total
    records = []
    for k, i in enumerate(mols):
        if k in between:
            running = between[k](st, running)
        kind, com_new, atoms_new, ei = st.propose(i)
        forced = None
        if k in script:
            sc = script[k]
            forced = sc.get("accept")
            if "mol" in sc:
                (st.trans if kind == "trans" else st.rot).attempt -= 1   # the draw is not made
                i, com_new, atoms_new = sc["mol"], np.asarray(sc["com"], float), np.asarray(sc["atoms"], float)
                kind, ei = "scripted", st.quat[i - 1]
        ref = lockstep.move(i, com_new, atoms_new) if lockstep is not None else None
        got = form.move(i, com_new, atoms_new)
        what = f"move {k} (molecule {i}, {kind})"
        if ref is not None:
            if "d" in got:
                lockstep.check_d(got["d"], got["overlap"], ref, what)
            else:
                lockstep.check_calls(got, ref, what)
        delta, u = got["delta"], None
        if got["overlap"]:
            accepted = False                                                  # :598
        elif forced is not None:
            accepted = forced
        elif delta / T < 0.0:                                                 # Metropolis
            accepted = True
        else:
            u = st.rng.random()
            accepted = math.exp(-delta / T) > u
        if ref is not None:
            lockstep.note_decision(ref["delta"], u, what)
        form.settle(accepted)
        if ref is not None:
            lockstep.settle(accepted)
        if accepted:
            if running is not None:
                running += delta                                             # :599
            if kind == "trans":
                st.trans.naccept += 1
            elif kind == "rot":
                st.rot.naccept += 1
            if kind != "scripted":
                st.quat[i - 1] = ei                                          # :620
            if ref is not None and form.s_old() is not None:
                lockstep.check_s_old(form.s_old(), what)
        records.append((i, kind, bool(accepted), bool(got["overlap"]), _values(got)))
        if adjust_every and (k + 1) % adjust_every == 0:
            st.adjust()
        if check_total is not None and block and (k + 1) % block == 0:
            check_total(st, running, k)
    if check_total is not None and (not block or n_moves % block):
        check_total(st, running, n_moves - 1)
    if lockstep is not None and lockstep.close_calls:
        warnings.warn("Loop() replay:" + lockstep.report())
    return running, records


def _values(got):
    if "d" in got:
        return np.concatenate([np.asarray(got["d"], float), [got["delta"]]])
    return np.array([*got["lj_old"], *got["q_old"][:2], *got["lj_new"], *got["q_new"][:2],
                     got["recip"], got["delta"]], dtype=float)


# ---- scripted moves ---------------------------------------------------------------------------------
def overlap_move(st, i):
    """Molecule i translated rigidly so that its first atom sits 0.3 A from the last atom of the
    molecule whose centre is nearest (opposite charges for water: O on H): an overlap for
    EwaldShort (r^2 < 0.5, ewalds.jl:359) and CoulombReal (r^2 < 1, energy.jl:695)."""
    com = st.moa.COM
    d = com - com[i - 1]
    d -= st.box * np.round(d / st.box)
    r2 = (d * d).sum(1)
    r2[i - 1] = np.inf
    j = int(np.argmin(r2)) + 1
    fj, lj = st.span(j)
    fi, _ = st.span(i)
    target = st.soa.coords[lj - 1] + np.array([0.3, 0.0, 0.0])
    shift = target - st.soa.coords[fi]
    return dict(mol=i, com=st.moa.COM[i - 1] + shift, atoms=st.atoms(i) + shift)


def zero_move(st, i, accept):
    """A move that puts molecule i where it is: RecipMove's dS is exactly zero, so sumQExpNew
    equals sumQExpOld bit for bit whichever way the move is decided."""
    return dict(mol=i, com=st.moa.COM[i - 1].copy(), atoms=st.atoms(i), accept=accept)
