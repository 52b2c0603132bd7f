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


def parts_at(orc, a, f, kappa, rcut, qq_rcut=None):
    """The four parts of U at scale f and whether any molecule overlaps there (EwaldReal's sentinel,
    ewalds.jl:359-360, molecule by molecule).  rcut is the LJ cutoff and, unless qq_rcut is given,
    the Coulomb cutoff too."""
    qq_rcut = rcut if qq_rcut is None else qq_rcut
    alpha = kappa * a["box"]
    a2 = host_rescale(a, f)
    s = common.oracle_system(a2)
    kap = alpha / a2["box"]
    t = orc.potential_ewald(s, orc.Ewald(kap, 5, 27, a2["box"]), rcut, qq_rcut)
    ovl = any(orc.ewald_real(i, s, kap, qq_rcut)[1] for i in range(1, a2["com"].shape[0] + 1))
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


def perturb(orc, a, scales, kappa, rcut, temperature, qq_rcut=None):
    """One replica: dict(base [4], du [K, 4], ovl [K], w [K], ovl0); an overlap at f = 1 (ovl0) holds for
    every k."""
    base, o0 = parts_at(orc, a, 1.0, kappa, rcut, qq_rcut)
    du, ovl = [], []
    for f in scales:
        u, o = parts_at(orc, a, float(f), kappa, rcut, qq_rcut)
        du.append(u - base)
        ovl.append(o or o0)
    du, ovl = np.array(du), np.array(ovl)
    w, z = weights(du, ovl, scales, a["com"].shape[0], temperature)
    return dict(base=base, du=du, ovl=z, w=w, ovl0=bool(o0))


def host_sums(du, zero, scales, n_mol, temperature, boltz0, novl0):
    """What one call adds to the accumulators, from the call's own du [R, K, 4]."""
    w, z = weights(du, zero, scales, n_mol, temperature)
    return np.asarray(boltz0, dtype=float) + w, np.asarray(novl0, dtype=np.int64) + z


def overlap_case(a, mol_i=0, mol_j=1, r2=0.52, atom_i=0):
    """`a` with molecule mol_j translated so that its first hydrogen sits at r^2 = r2 from the oxygen
    of mol_i ALONG the COM-COM axis: with u = COM_j - COM_i the pair vector is H_j - O_i = sigma u/|u|
    and a rescale by f makes it (sigma + (f - 1) |u|) u/|u|.  Solving H_j - O_i = u + g, g = (H_j -
    COM_j) - (O_i - COM_i), gives u = -(|g| + sigma) g/|g|.  Returns (arrays, |u|).  (atom_i: the atom
    of mol_i to approach in place of its oxygen.)"""
    com, coords = a["com"].copy(), a["coords"].copy()
    sigma = np.sqrt(r2)
    g = (coords[3 * mol_j + 1] - com[mol_j]) - (coords[3 * mol_i + atom_i] - com[mol_i])
    ng = np.linalg.norm(g)
    u = -(ng + sigma) * g / ng
    t = (com[mol_i] + u) - com[mol_j]
    com[mol_j] += t
    coords[3 * mol_j:3 * mol_j + 3] += t
    return dict(a, com=com, coords=coords), float(ng + sigma)


def contact_case(a, mol_i=0, mol_j=1, r2=0.2):
    """overlap_case for a LIKE-charge pair: the first hydrogen of mol_j at r^2 = r2 < 0.25 from the
    first hydrogen of mol_i along the COM-COM axis -- below the erfc table's first node, where the
    pair is evaluated by the series in kappa_k r, and no overlap (the charges have one sign).
    Returns (arrays, |u|)."""
    return overlap_case(a, mol_i, mol_j, r2, atom_i=1)


def pair_r2(a, f, mol_i, atom_i, mol_j, atom_j):
    """r^2 of one atom pair (minimum image) after the rescale by f."""
    a2 = host_rescale(a, f)
    d = a2["coords"][3 * mol_j + atom_j] - a2["coords"][3 * mol_i + atom_i]
    d -= a2["box"] * np.round(d / a2["box"])
    return float(d @ d)


def min_r2_opposite(a, f):
    """The smallest r^2 (minimum image) over atom pairs of different molecules with opposite charges,
    after the rescale by f."""
    a2 = host_rescale(a, f)
    x, q, L = a2["coords"], np.asarray(a2["charge"]), a2["box"]
    d = x[:, None, :] - x[None, :, :]
    d -= L * np.round(d / L)
    r2 = np.einsum("ijk,ijk->ij", d, d)
    mol = np.arange(x.shape[0]) // 3
    m = (mol[:, None] != mol[None, :]) & (q[:, None] * q[None, :] < 0)
    return float(r2[m].min())


def prefix(a, n_mol):
    """The first n_mol molecules of `a` (3 atoms each) in the same box."""
    out = dict(a, com=a["com"][:n_mol].copy(), coords=a["coords"][:3 * n_mol].copy(),
               atype=a["atype"][:3 * n_mol].copy(), charge=a["charge"][:3 * n_mol].copy())
    for k in ("first_atom", "last_atom"):
        if k in a:
            out[k] = a[k][:n_mol].copy()
    return out


def domain_ok(box, rcut, scales, alpha=5.6):
    """mmc_batch_volume_perturb's own conditions on (box, r_cut, scales): every test box >= 2 r_cut
    and (kappa, r_cut) at the smallest one inside the erfc table's domain (include/mmc_hip.h)."""
    l_min = min(min(scales), 1.0) * box
    kappa = alpha / l_min
    return (l_min >= 2 * rcut and kappa <= 0.5 and rcut * rcut + 100 <= 256.0
            and kappa * np.sqrt(rcut * rcut + 100) <= 4.0)


def dense_prefix(n_mol, n_full=300):
    """The first n_mol molecules of a dense SPC/E lattice of n_full (test_gpu_batch._dense_water) in
    the box of the n_full: 20.85 A at 300, so that r_cut = 9 fits a box compressed by 0.95."""
    from test_gpu_batch import _dense_water
    return prefix(_dense_water(n_full), n_mol)


def lj9_system():
    """The three-type model of test_gpu_batch.test_fast_kernel_with_several_lj_pairs_per_molecule_pair:
    150 identical molecules whose three sites all carry LJ (nine LJ atom pairs per molecule pair)."""
    a = common.random_system(150, 24.0, seed=31, na_choices=(3,), n_types=3)
    n_mol = a["com"].shape[0]
    a["atype"] = np.tile([1, 2, 3], n_mol).astype(np.int64)
    a["charge"] = np.tile(np.array([-0.8, 0.5, 0.3]), n_mol)
    e, s = np.array([60.0, 25.0, 8.0]), np.array([3.1, 2.6, 2.2])
    a["eps"], a["sig"] = np.sqrt(e[:, None] * e[None, :]), (s[:, None] + s[None, :]) / 2
    return a


def shifted_states(a, n):
    """n configurations distinct from `a` and from each other: the whole system translated (and
    wrapped by COM), one molecule more."""
    L = float(a["box"])
    out = []
    for k in range(n):
        shift = np.array([1.3 + 0.7 * k, -2.1 + 0.4 * k, 0.4 - 0.9 * k])
        com = (a["com"] + shift) % L
        coords = a["coords"] + np.repeat(com - a["com"], 3, axis=0)
        m = k % a["com"].shape[0]
        d = np.array([0.3, 0.2, -0.1]) * (1 + 0.5 * k)
        com[m] += d
        coords[3 * m:3 * m + 3] += d
        out.append(dict(a, com=com, coords=coords))
    return out
