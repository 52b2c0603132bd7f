"""mmc_batch_volume_perturb restated in numpy on top of the oracle (include/mmc_hip.h, "Virtual
volume moves"): the NPT move's rescale (volumeChange.jl:62-80) by f on the host, the oracle's
potential(..., "ewald") in box L_k = f L with kappa_k = alpha / L_k, alpha = kappa L, the part
differences against the same evaluation at f = 1, the weights, and the overlap rule."""
import numpy as np

import common

PARTS = ("lj", "real", "recip", "self")


def host_rescale(a, f):
    """k_rescale's arithmetic: per COM component new = old * f, d = new - old, every atom + d."""
    com = a["com"] * f
    d = com - a["com"]
    return dict(a, com=com, coords=a["coords"] + np.repeat(d, 3, axis=0), box=float(f * a["box"]))


def scale_of_dv(box, dv):
    """volumeChange.jl:60 for a volume change dv: L'/L = ((V + dv) / V) ** (1 / 3)."""
    v = box ** 3
    return ((v + dv) / v) ** (1.0 / 3.0)


def parts_at(orc, a, f, kappa, rcut):
    """The four parts of U at scale f and whether any molecule overlaps there (EwaldReal's sentinel,
    ewalds.jl:359-360, molecule by molecule)."""
    alpha = kappa * a["box"]
    a2 = host_rescale(a, f)
    s = common.oracle_system(a2)
    kap = alpha / a2["box"]
    t = orc.potential_ewald(s, orc.Ewald(kap, 5, 27, a2["box"]), rcut, rcut)
    ovl = any(orc.ewald_real(i, s, kap, rcut)[1] for i in range(1, a2["com"].shape[0] + 1))
    return np.array([t[k] for k in PARTS]), ovl


def weights(du, zero, scales, n_mol, temperature):
    """w = exp(-dU / T + N ln(scale^3)), dU = ((dLJ + dreal) + drecip) + dself; 0 where `zero` or dU
    is not finite.  du [..., K, 4], zero [..., K].  Returns (w, forced to zero)."""
    sc = np.asarray(scales, dtype=float)
    with np.errstate(over="ignore", invalid="ignore"):
        d = ((du[..., 0] + du[..., 1]) + du[..., 2]) + du[..., 3]
        z = np.asarray(zero, dtype=bool) | ~np.isfinite(d)
        w = np.exp(-d / temperature + float(n_mol) * np.log(sc * sc * sc))
    return np.where(z, 0.0, w), z


def perturb(orc, a, scales, kappa, rcut, temperature):
    """One replica: dict(base [4], du [K, 4], ovl [K], w [K]); an overlap at f = 1 holds for every k."""
    base, o0 = parts_at(orc, a, 1.0, kappa, rcut)
    du, ovl = [], []
    for f in scales:
        u, o = parts_at(orc, a, float(f), kappa, rcut)
        du.append(u - base)
        ovl.append(o or o0)
    du, ovl = np.array(du), np.array(ovl)
    w, z = weights(du, ovl, scales, a["com"].shape[0], temperature)
    return dict(base=base, du=du, ovl=z, w=w)


def host_sums(du, zero, scales, n_mol, temperature, boltz0, novl0):
    """What one call adds to the accumulators, from the call's own du [R, K, 4]."""
    w, z = weights(du, zero, scales, n_mol, temperature)
    return np.asarray(boltz0, dtype=float) + w, np.asarray(novl0, dtype=np.int64) + z


def overlap_case(a, mol_i=0, mol_j=1, r2=0.52):
    """`a` with molecule mol_j translated so that its first hydrogen sits at r^2 = r2 from the oxygen
    of mol_i ALONG the COM-COM axis: with u = COM_j - COM_i the pair vector is H_j - O_i = sigma u/|u|
    and a rescale by f makes it (sigma + (f - 1) |u|) u/|u|.  Solving H_j - O_i = u + g, g = (H_j -
    COM_j) - (O_i - COM_i), gives u = -(|g| + sigma) g/|g|.  Returns (arrays, |u|)."""
    com, coords = a["com"].copy(), a["coords"].copy()
    sigma = np.sqrt(r2)
    g = (coords[3 * mol_j + 1] - com[mol_j]) - (coords[3 * mol_i] - com[mol_i])
    ng = np.linalg.norm(g)
    u = -(ng + sigma) * g / ng
    t = (com[mol_i] + u) - com[mol_j]
    com[mol_j] += t
    coords[3 * mol_j:3 * mol_j + 3] += t
    return dict(a, com=com, coords=coords), float(ng + sigma)
