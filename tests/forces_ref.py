"""Restatement in numpy fp64 of the forces mmc_batch_forces defines (include/mmc_hip.h, "Forces and
torques"), from a replica's (com, coords, S) as Batch.get_replica returns them, and the fixed-order
sums of k_forces_reduce on the host.  Beside each output stands A, the same sum taken over the
absolute values of its terms: the scale the GPU tests' tolerance is a multiple of.  Not a test
module."""
import numpy as np

from deletion_ref import wave_sum_rows


def vector1D(c1, c2, box):
    """boundaries.jl:8-14 on arrays: c2 - c1, moved by one box where |c2 - c1| >= box / 2."""
    d = np.asarray(c2, dtype=np.float64) - np.asarray(c1, dtype=np.float64)
    m = np.where(np.abs(d) < 0.5 * box, 0.0, np.copysign(1.0, d))
    return d - m * box


def erfc(x):
    import math
    return np.vectorize(math.erfc, otypes=[np.float64])(x)


def setup(a, orc, box, lj_rcut, qq_rcut, alpha=5.6):
    """What every molecule of one system shares: the k list of the reference, the tables of the
    molecule's three slots and the cutoffs."""
    from metropolismontecarlo_amd import structs
    L = float(box)
    ew = orc.Ewald(alpha / L, 5, 27, L, factor=structs.factor)
    ty = np.asarray(a["atype"][:3], dtype=np.int64) - 1
    return {"box": L, "kappa": alpha / L, "factor": float(structs.factor),
            "kxyz": ew.kxyz.astype(np.float64), "cfac": ew.cfac.copy(),
            "q": np.asarray(a["charge"][:3], dtype=np.float64),
            "eps": np.asarray(a["eps"], dtype=np.float64)[np.ix_(ty, ty)],
            "sig": np.asarray(a["sig"], dtype=np.float64)[np.ix_(ty, ty)],
            "lj_gate": lj_rcut * lj_rcut, "qq_gate": qq_rcut * qq_rcut,
            "lj_slack": lj_rcut * lj_rcut + 100, "qq_slack": qq_rcut * qq_rcut + 100}


def reciprocal(su, coords, S, i):
    """(f [3, 3], A [3, 3]): factor (4 pi / L) q_a sum_k cfac_k n_k Im(conj(S_k) e_{a,k}) of the
    three atoms of molecule i, over the reference's k list (kx >= 0, doubled weights for kx > 0)."""
    L = su["box"]
    x = np.asarray(coords, dtype=np.float64)[3 * i:3 * i + 3]
    e = np.exp(2j * np.pi * (su["kxyz"] @ x.T) / L)                          # [k, a]
    S = np.asarray(S).ravel()
    im = S.real[:, None] * e.imag - S.imag[:, None] * e.real                  # Im(conj(S) e)
    ab = np.abs(S.real[:, None] * e.imag) + np.abs(S.imag[:, None] * e.real)
    w = su["cfac"][:, None] * su["kxyz"]                                      # [k, d]
    pre = su["factor"] * (4.0 * np.pi / L) * su["q"]
    f = pre[:, None] * np.einsum("ka,kd->ad", im, w)
    A = np.abs(pre)[:, None] * np.einsum("ka,kd->ad", ab, np.abs(w))
    return f, A


def molecule(su, com, coords, S, i, mass=None):
    """Every output of molecule i (0-based) and its A.  Returns a dict: atom [3, 3], force [3],
    torque [3], vir [3] = (w_lj, w_real, t), each with an "A_" twin; overlap (bool); recip [3, 3]
    (the reciprocal part of atom alone); image_margin and r_margin (how far, in A, the counted atom
    pairs are from flipping their image and from r^2 = 0.25, 0.5 and the slack); gate_margin (the
    smallest | |rij| - r_gate | over the other molecules: how far the nearest COM is from flipping a
    gate); pair_min (the smallest atom-pair
    r^2 inside the gate)."""
    L, kappa, factor = su["box"], su["kappa"], su["factor"]
    com, coords = np.asarray(com, dtype=np.float64), np.asarray(coords, dtype=np.float64)
    n = com.shape[0]
    at = coords.reshape(n, 3, 3)
    others = np.arange(n) != i
    rij = vector1D(com[i][None, :], com, L)                                   # [j, d]
    rij2 = rij[:, 0] * rij[:, 0] + rij[:, 1] * rij[:, 1] + rij[:, 2] * rij[:, 2]
    gq, gl = others & (rij2 < su["qq_gate"]), others & (rij2 < su["lj_gate"])
    rab = vector1D(at[i][None, :, None, :], at[:, None, :, :], L)             # [j, a, b, d]
    r2 = rab[..., 0] * rab[..., 0] + rab[..., 1] * rab[..., 1] + rab[..., 2] * rab[..., 2]
    qq = su["q"][:, None] * su["q"][None, :]                                  # [a, b]
    safe = np.where(r2 > 0, r2, 1.0)
    # real-space Ewald (ewalds.jl:359-367)
    ovl_pair = gq[:, None, None] & (r2 < 0.5) & (qq[None] < 0)
    on_q = gq[:, None, None] & ~ovl_pair & (r2 < su["qq_slack"])
    cq = np.zeros_like(r2)
    u = safe[on_q]
    r = np.sqrt(u)
    cq[on_q] = factor * np.broadcast_to(qq[None], r2.shape)[on_q] \
        * (erfc(kappa * r) / r + 2.0 * kappa / np.sqrt(np.pi) * np.exp(-kappa * kappa * u)) / u
    # Lennard-Jones (energy.jl:270-281)
    eps, sig = su["eps"][None], su["sig"][None]
    on_l = gl[:, None, None] & (r2 < su["lj_slack"]) & (eps > 0.001)
    s2 = sig * sig / safe
    s6 = s2 * s2 * s2
    s12 = s6 * s6
    virab = eps * (2.0 * s12 - s6)
    cl = np.where(on_l, 24.0 * virab / safe, 0.0)
    fab_ref = np.where(on_l[..., None], rab * (virab * s2)[..., None], 0.0)   # the reference's own fab
    f_pair = -((cq + cl)[..., None] * rab).sum(axis=(0, 2))                   # [a, d]
    A_pair = ((np.abs(cq) + np.abs(cl))[..., None] * np.abs(rab)).sum(axis=(0, 2))
    f_rec, A_rec = reciprocal(su, coords, S, i)
    f, A = f_pair + f_rec, A_pair + A_rec
    d = vector1D(com[i][None, :], at[i], L)                                   # [a, d]
    F, AF = (f[0] + f[1]) + f[2], A.sum(0)
    tau = np.cross(d, f).sum(0)
    ad = np.abs(d)
    A_tau = np.stack([ad[:, 1] * A[:, 2] + ad[:, 2] * A[:, 1], ad[:, 2] * A[:, 0] + ad[:, 0] * A[:, 2],
                      ad[:, 0] * A[:, 1] + ad[:, 1] * A[:, 0]], axis=1).sum(0)
    w_terms = rij[:, None, None, :] * fab_ref                                 # [j, a, b, d]
    w_lj, A_wlj = w_terms.sum() * 24 / 3.0, np.abs(w_terms).sum() * 24 / 3.0
    g_terms = rij[:, None, None, :] * (cq[..., None] * rab)
    w_real, A_wreal = g_terms.sum() / 3.0, np.abs(g_terms).sum() / 3.0
    t, A_t = 0.0, 0.0
    if mass is not None:
        m = np.asarray(mass, dtype=np.float64)
        I = np.zeros((3, 3))
        for a in range(3):
            I += m[a] * ((d[a] @ d[a]) * np.eye(3) - np.outer(d[a], d[a]))
        with np.errstate(all="ignore"):
            cof, A_cof = np.zeros((3, 3)), np.zeros((3, 3))
            for p in range(3):
                for q in range(3):
                    p1, p2, q1, q2 = (p + 1) % 3, (p + 2) % 3, (q + 1) % 3, (q + 2) % 3
                    cof[p, q] = I[p1, q1] * I[p2, q2] - I[p1, q2] * I[p2, q1]
                    A_cof[p, q] = abs(I[p1, q1] * I[p2, q2]) + abs(I[p1, q2] * I[p2, q1])
            det = (I[0] * cof[0]).sum()
            A_det = (np.abs(I[0]) * A_cof[0]).sum()
            t = float(tau @ cof @ tau / det)          # (I is symmetric: the cofactor matrix is its own transpose)
            A_t = float(A_tau @ A_cof @ A_tau / abs(det) * (A_det / abs(det)))
    inside = np.concatenate([r2[gq].ravel(), r2[gl].ravel()])
    gated = gq | gl
    raw = np.abs(at[gated][:, None, :, :] - at[i][None, :, None, :])          # before the image is taken
    image_margin = float(np.abs(raw - 0.5 * L).min()) if gated.any() else np.inf
    thr = np.array([0.25, 0.5, su["qq_slack"], su["lj_slack"]])
    r_margin = float(np.abs(np.sqrt(inside)[:, None] - np.sqrt(thr)[None, :]).min()) if inside.size else np.inf
    gates = np.sqrt(np.array([su["qq_gate"], su["lj_gate"]]))
    margin = np.abs(np.sqrt(rij2[others])[:, None] - gates[None, :]).min()
    return {"atom": f, "A_atom": A, "force": F, "A_force": AF, "torque": tau, "A_torque": A_tau,
            "vir": np.array([w_lj, w_real, t]), "A_vir": np.array([A_wlj, A_wreal, A_t]),
            "overlap": bool(ovl_pair.any()), "recip": f_rec, "A_recip": A_rec,
            "gate_margin": float(margin), "pair_min": float(inside.min()) if inside.size else np.inf,
            "image_margin": image_margin, "r_margin": r_margin, "d": d}


def fd_safe(ref, step):
    """Whether moving molecule i's atoms by up to `step` keeps every counted atom pair on its image
    and on its side of r^2 = 0.25, 0.5 and the slack: what a finite difference of the oracle needs
    (ref: molecule()'s dict)."""
    return ref["image_margin"] > 4 * step and ref["r_margin"] > 4 * step


def close(x, ref, A):
    """The GPU tests' tolerance per value: 1e-12 A + 1e-300."""
    return bool(np.all(np.abs(np.asarray(x) - np.asarray(ref)) <= 1e-12 * np.asarray(A) + 1e-300))


def check(su, b, r, sel, out, rows, mass=None, what="", refs=None):
    """Every output of replica r's selected molecules sel (out: Batch.forces' dict with details,
    rows: where molecule sel[k] sits in its arrays) against `molecule` on the replica's own
    coordinates and S(k) (refs: those dicts, where the caller has them already).  Returns the worst
    |x - ref| / A seen (for the record)."""
    com, coords, S = b.get_replica(r)
    bad, worst = [], 0.0
    for q, (k, i) in enumerate(zip(rows, sel)):
        ref = molecule(su, com, coords, S, int(i), mass) if refs is None else refs[q]
        if bool(out["ovl"][r, k] & 1) != ref["overlap"]:
            bad.append((int(i), "overlap", int(out["ovl"][r, k]), ref["overlap"]))
            continue
        if ref["overlap"]:                           # (a flagged molecule's rows are zeros)
            continue
        for name in ("atom", "force", "torque", "vir"):
            x, A = out[name][r, k], ref["A_" + name]
            err = np.abs(x - ref[name])
            with np.errstate(all="ignore"):
                worst = max(worst, float(np.nanmax(np.where(A > 0, err / A, 0.0))))
            if not close(x, ref[name], A):
                bad.append((int(i), name, x.tolist(), ref[name].tolist(), (err / (A + 1e-300)).max()))
    assert not bad, f"{what} replica {r}: {bad[:4]}"
    return worst


def host_sums(force, torque, vir, ovl, nflag0=None):
    """k_forces_reduce on the host, from the returned rows force, torque, vir [R, n, 3] and flags ovl
    [R, n]: lane l adds the replica's unflagged entries l, l + 64, ... in that order -- 1.0, F.F,
    tau.tau, t, F_x, F_y, F_z, w_lj, w_real, every product (x x + y y) + z z -- and the 64 lane sums
    go through wave_sum_rows.  Returns (fsum [R, 9], n_flagged [R])."""
    force, torque, vir = (np.asarray(x, dtype=np.float64) for x in (force, torque, vir))
    ovl = np.asarray(ovl)
    R, n = ovl.shape
    fsum = np.zeros((R, 9))
    nfl = np.zeros(R, dtype=np.int64) if nflag0 is None else np.array(nflag0, dtype=np.int64).copy()
    for r in range(R):
        acc = np.zeros((9, 64))
        for e in range(n):
            if ovl[r, e]:
                continue
            lane = e % 64
            f, t, w = force[r, e], torque[r, e], vir[r, e]
            acc[0, lane] += 1.0
            acc[1, lane] += (f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]
            acc[2, lane] += (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]
            acc[3, lane] += w[2]
            acc[4, lane] += f[0]
            acc[5, lane] += f[1]
            acc[6, lane] += f[2]
            acc[7, lane] += w[0]
            acc[8, lane] += w[1]
        for q in range(9):
            fsum[r, q] = wave_sum_rows(acc[q])
        nfl[r] += int(np.count_nonzero(ovl[r]))
    return fsum, nfl
