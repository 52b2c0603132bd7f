"""Host-side counterparts of the reference types that cross the hot-path boundary.

Field names are the reference's (Ewald/ewalds.jl:9-19, Ewald/auxillary.jl:37-91,
Ewald/structs.jl:283-347).  Julia identifiers that are not ASCII keep an ASCII alias:
``Tables.eps_ij`` is ``Tables.ϵᵢⱼ``, ``Properties2.rho`` is ``ρ``.  Arrays are numpy: a
``Vector{SVector{3,Float64}}`` is an (n, 3) float64 array, index arrays keep Julia's 1-based
values.
"""
import math
from dataclasses import dataclass, field

import numpy as np


# Ewald/constants.jl:24-28 (same order of operations -> same double)
def _factor():
    kb1 = 1.3806488e-23
    eps01 = 8.854187817e-12
    eps01 *= 1e-10
    e1 = 1.602176565e-19
    return e1 ** 2 / eps01 / 4 / math.pi / kb1


factor = _factor()
R = 8.3144621e-3  # kJ mol^-1 K^-1, Ewald/constants.jl:11


class StructArray:
    """Minimal stand-in for StructArrays.StructArray: one numpy column per field, the way the
    hot path reads it (`moa.COM`, `moa.firstAtom`, `soa.coords`, `soa.charge`, `soa.atype`)."""

    def __init__(self, **columns):
        n = None
        for k, v in columns.items():
            v = np.asarray(v)
            n = len(v) if n is None else n
            if len(v) != n:
                raise ValueError(f"column {k} has length {len(v)}, expected {n}")
            setattr(self, k, v)
        self._names = list(columns)
        self._n = n or 0

    def __len__(self):
        return self._n


def make_moa(COM, firstAtom, lastAtom, molType=None):
    """moa: ParticleAtomKMC/Molecule columns used by the path (Ewald/structs.jl:314-321)."""
    COM = np.ascontiguousarray(COM, dtype=np.float64).reshape(-1, 3)
    n = COM.shape[0]
    return StructArray(COM=COM, firstAtom=np.ascontiguousarray(firstAtom, dtype=np.int64),
                       lastAtom=np.ascontiguousarray(lastAtom, dtype=np.int64),
                       molType=np.ones(n, dtype=np.int64) if molType is None else
                       np.asarray(molType, dtype=np.int64))


def make_soa(coords, atype, charge, molNum=None):
    """soa: atom columns used by the path (Ewald/structs.jl:283-290)."""
    coords = np.ascontiguousarray(coords, dtype=np.float64).reshape(-1, 3)
    n = coords.shape[0]
    return StructArray(coords=coords, atype=np.ascontiguousarray(atype, dtype=np.int64),
                       charge=np.ascontiguousarray(charge, dtype=np.float64),
                       molNum=np.zeros(n, dtype=np.int64) if molNum is None else
                       np.asarray(molNum, dtype=np.int64))


class Tables:
    """Ewald/structs.jl:337-347: eps_ij = sqrt(eps_i eps_j), sig_ij = (sig_i + sig_j)/2."""

    def __init__(self, a, b):
        a = np.asarray(a, dtype=np.float64)
        b = np.asarray(b, dtype=np.float64)
        self.eps_ij = np.sqrt(a[:, None] * a[None, :])
        self.sig_ij = (b[:, None] + b[None, :]) / 2

    ϵᵢⱼ = property(lambda s: s.eps_ij, lambda s, v: setattr(s, "eps_ij", np.asarray(v, float)))
    σᵢⱼ = property(lambda s: s.sig_ij, lambda s, v: setattr(s, "sig_ij", np.asarray(v, float)))


class Solute:
    """A rigid foreign solute of S sites for Batch.widom_solute (include/mmc_hip.h, "Foreign
    solutes"): offsets (S, 3) A from its reference point, charge (S,), and eps / sig (S, 3) in K and
    A against the three atom slots of the batch's molecule, already mixed (the Tables entries
    eps_ij[type_a, type_slot]).  The reference has no such struct: it is the argument block of
    mmc_batch_widom_solute."""
    MAX_SITES = 16  # MMC_SOLUTE_MAX_SITES

    def __init__(self, name, offsets, charge, eps, sig):
        self.name = str(name)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.float64).reshape(-1, 3)
        S = self.offsets.shape[0]
        self.charge = np.ascontiguousarray(charge, dtype=np.float64).reshape(S)
        self.eps = np.ascontiguousarray(eps, dtype=np.float64).reshape(S, 3)
        self.sig = np.ascontiguousarray(sig, dtype=np.float64).reshape(S, 3)
        if not 1 <= S <= self.MAX_SITES:
            raise ValueError(f"a solute has 1..{self.MAX_SITES} sites, not {S}")

    @property
    def n_sites(self):
        return self.offsets.shape[0]

    def __repr__(self):
        return f"Solute({self.name!r}, {self.n_sites} sites, net charge {self.charge.sum():+.4f})"


class SolutePair:
    """Two rigid foreign solutes for Batch.widom_pair (include/mmc_hip.h, "Solute pairs"): Solute a,
    Solute b and their cross table eps_ab / sig_ab (S_A, S_B) in K and A, already mixed.  S_A + S_B
    may not exceed Solute.MAX_SITES."""
    MAX_SEP = 32  # MMC_PAIR_MAX_SEP

    def __init__(self, a, b, eps_ab, sig_ab):
        if not isinstance(a, Solute) or not isinstance(b, Solute):
            raise ValueError("a and b must be Solutes")
        self.a, self.b = a, b
        self.eps_ab = np.ascontiguousarray(eps_ab, dtype=np.float64).reshape(a.n_sites, b.n_sites)
        self.sig_ab = np.ascontiguousarray(sig_ab, dtype=np.float64).reshape(a.n_sites, b.n_sites)
        if a.n_sites + b.n_sites > Solute.MAX_SITES:
            raise ValueError(f"a solute pair has at most {Solute.MAX_SITES} sites in all, not "
                             f"{a.n_sites} + {b.n_sites}")
        for name, t in (("eps_ab", self.eps_ab), ("sig_ab", self.sig_ab)):
            if not np.all(np.isfinite(t)) or np.any(t < 0):
                raise ValueError(f"{name} must be finite and >= 0")

    def swapped(self):
        """The pair with A and B exchanged."""
        return SolutePair(self.b, self.a, self.eps_ab.T, self.sig_ab.T)

    def __repr__(self):
        return f"SolutePair({self.a.name!r}, {self.b.name!r})"


class EWALD:
    """mutable struct EWALD{I} (Ewald/ewalds.jl:9-19)."""

    def __init__(self, kappa, nk, k_sq_max, NKVECS, kxyz, cfac, sumQExpOld, sumQExpNew, factor):
        self.kappa = float(kappa)
        self.nk = int(nk)
        self.k_sq_max = int(k_sq_max)
        self.NKVECS = int(NKVECS)
        self.kxyz = np.asarray(kxyz, dtype=np.int32)
        self.cfac = np.asarray(cfac, dtype=np.float64)
        self.sumQExpOld = np.asarray(sumQExpOld, dtype=np.complex128)
        self.sumQExpNew = np.asarray(sumQExpNew, dtype=np.complex128)
        self.factor = float(factor)


@dataclass
class Properties:
    """Ewald/auxillary.jl:37-45"""
    energy: float = 0.0
    virial: float = 0.0
    coulomb: float = 0.0
    recip: float = 0.0
    recipOld: float = 0.0
    old_e: float = 0.0
    old_v: float = 0.0


@dataclass
class Moves:
    """Ewald/auxillary.jl:48-55"""
    naccepp: int = 0
    naccept: int = 0
    attempp: int = 0
    attempt: int = 0
    set_value: float = 0.5
    d_max: float = 0.0


@dataclass
class Properties2:
    """Ewald/auxillary.jl:78-91 (rho = the reference's field `ρ`, dphi_max = `dϕ_max`)."""
    temperature: float = 298.15
    rho: float = 0.0
    pressure: float = 0.0
    dr_max: float = 0.0
    dphi_max: float = 0.0
    move_accept: float = 0.3
    numTranAccepted: int = 0
    totalStepsTaken: int = 0
    quat: list = field(default_factory=list)
    LJ_rcut: float = 10.0
    qq_rcut: float = 10.0
    box: float = 0.0


@dataclass
class Requirements:
    """Legacy argument bundle (Ewald/auxillary.jl:59-75)."""
    rm: np.ndarray
    ra: np.ndarray
    nMols: int
    nAtoms: int
    nCharges: int
    thisMol_theseAtoms: np.ndarray  # (n_mol, 2) 1-based inclusive
    molNames: list
    molTypes: list
    atomNames: list
    atomTypes: np.ndarray
    table: Tables
    box: float
    r_cut: float
