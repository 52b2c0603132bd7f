"""Restatement in numpy fp64 of every output of mmc_batch_solute_forces (include/mmc_hip.h, "A fixed
solute: the mean force, field and potential on it") for one replica, from its (com, coords, S) as
Batch.get_replica returns them and the solute as it was set.  Beside each output stands A_, the same sum
taken over the absolute values of its terms: the scale the GPU tests' tolerance is a multiple of
(forces_ref.molecule does the same for mmc_batch_forces).  Not a test module."""
import numpy as np

from forces_ref import close, erfc, setup, vector1D  # noqa: F401  (setup, close: for the tests)


def _r2(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def reciprocal(su, sites, S):
    """(rec [S, 4], A [S, 4]): the reciprocal field factor (4 pi / L) sum_k cfac_k n_k Im(conj(S_k) e_{a,k})
    and potential 2 factor sum_k cfac_k Re(conj(S_k) e_{a,k}) at the sites, over the reference's k list."""
    L, factor = su["box"], su["factor"]
    e = np.exp(2j * np.pi * (su["kxyz"] @ np.asarray(sites, dtype=np.float64).T) / L)      # [k, a]
    S = np.asarray(S).ravel()
    im = S.real[:, None] * e.imag - S.imag[:, None] * e.real                                # Im(conj(S) e)
    re = S.real[:, None] * e.real + S.imag[:, None] * e.imag                                # Re(conj(S) e)
    ab = np.abs(S.real[:, None] * e.imag) + np.abs(S.imag[:, None] * e.real)
    ab_re = np.abs(S.real[:, None] * e.real) + np.abs(S.imag[:, None] * e.imag)
    w = su["cfac"][:, None] * su["kxyz"]                                                    # [k, d]
    n = e.shape[1]
    rec, A = np.zeros((n, 4)), np.zeros((n, 4))
    rec[:, :3] = factor * (4.0 * np.pi / L) * np.einsum("ka,kd->ad", im, w)
    A[:, :3] = factor * (4.0 * np.pi / L) * np.einsum("ka,kd->ad", ab, np.abs(w))
    rec[:, 3] = 2.0 * factor * (su["cfac"][:, None] * re).sum(0)
    A[:, 3] = 2.0 * factor * (np.abs(su["cfac"])[:, None] * ab_re).sum(0)
    return rec, A


def replica(su, sol, mol, com, coords, S):
    """Every output of one replica and its A.  su: forces_ref.setup's dict; sol: the structs.Solute (its
    charge [S], eps, sig [S, 3]); mol [S + 1, 3]: the sites, then the reference point c.  Returns a dict:
    site_lj, field [S, 3], phi [S], recip [S, 4], site_force [S, 3], force, torque [3], each with an "A_"
    twin; real [S, 4] (the real-space part of field and phi) and self_phi [S] (the EwaldSelf term), so that
    real + recip + self = (field, phi); flags (bit 0 the overlap, bit 1 a non-finite output); d [S, 3];
    image_margin and r_margin (how far, in A, the counted atom pairs are from flipping their image and from
    r^2 = 0.25, 0.5 and the slacks); pair_min (the smallest counted r^2)."""
    L, kappa, factor = su["box"], su["kappa"], su["factor"]
    mol = np.asarray(mol, dtype=np.float64)
    ns = mol.shape[0] - 1
    sites, c = mol[:ns], mol[ns]
    q_s = np.asarray(sol.charge, dtype=np.float64)
    com = np.asarray(com, dtype=np.float64)
    n = com.shape[0]
    at = np.asarray(coords, dtype=np.float64).reshape(n, 3, 3)
    rij = vector1D(com, c[None, :], L)                                                      # [j, d]
    c2 = _r2(rij)
    gq, gl = c2 < su["qq_gate"], c2 < su["lj_gate"]   # the qq gate whether or not the solute is charged
    rab = vector1D(at[None, :, :, :], sites[:, None, None, :], L)                           # [a, j, b, d] site - atom
    r2 = _r2(rab)
    q_w = su["q"]
    qq = q_s[:, None, None] * q_w[None, None, :]                                            # [a, 1, b]
    with np.errstate(all="ignore"):
        ovl_pair = gq[None, :, None] & (r2 < 0.5) & (qq < 0)
        on_q = gq[None, :, None] & ~ovl_pair & (r2 < su["qq_slack"])
        r = np.sqrt(r2)
        e = np.where(on_q, erfc(kappa * r) / r, 0.0)
        fq = factor * np.broadcast_to(q_w[None, None, :], r2.shape)
        cq = np.where(on_q, fq * (e + 2.0 * kappa / np.sqrt(np.pi) * np.exp(-kappa * kappa * r2)) / r2, 0.0)
        ph = np.where(on_q, fq * e, 0.0)
        eps, sig = np.asarray(sol.eps, dtype=np.float64)[:, None, :], np.asarray(sol.sig, dtype=np.float64)[:, None, :]
        on_l = gl[None, :, None] & (r2 < su["lj_slack"]) & (eps > 0.001)
        s2 = sig * sig / r2
        s6 = s2 * s2 * s2
        s12 = s6 * s6
        cl = np.where(on_l, 24.0 * (eps * (2.0 * s12 - s6)) / r2, 0.0)
        site_lj = (cl[..., None] * rab).sum(axis=(1, 2))
        A_lj = (np.abs(cl)[..., None] * np.abs(rab)).sum(axis=(1, 2))
        real, A_real = np.zeros((ns, 4)), np.zeros((ns, 4))
        real[:, :3] = (cq[..., None] * rab).sum(axis=(1, 2))
        A_real[:, :3] = (np.abs(cq)[..., None] * np.abs(rab)).sum(axis=(1, 2))
        real[:, 3], A_real[:, 3] = ph.sum(axis=(1, 2)), np.abs(ph).sum(axis=(1, 2))
        rec, A_rec = reciprocal(su, sites, S)
        self_phi = -2.0 * factor * kappa / np.sqrt(np.pi) * q_s
        field, A_field = real[:, :3] + rec[:, :3], A_real[:, :3] + A_rec[:, :3]
        phi, A_phi = (real[:, 3] + rec[:, 3]) + self_phi, A_real[:, 3] + A_rec[:, 3] + np.abs(self_phi)
        f = site_lj + q_s[:, None] * field
        A_f = A_lj + np.abs(q_s)[:, None] * A_field
        d = vector1D(c[None, :], sites, L)
        F, A_F = f.sum(0), A_f.sum(0)
        tau = np.cross(d, f).sum(0)
        ad = np.abs(d)
        A_tau = np.stack([ad[:, 1] * A_f[:, 2] + ad[:, 2] * A_f[:, 1], ad[:, 2] * A_f[:, 0] + ad[:, 0] * A_f[:, 2],
                          ad[:, 0] * A_f[:, 1] + ad[:, 1] * A_f[:, 0]], axis=1).sum(0)
    finite = all(bool(np.all(np.isfinite(x))) for x in (site_lj, field, phi, rec, F, tau))
    flags = (1 if ovl_pair.any() else 0) | (0 if finite else 2)
    counted = on_q | on_l | ovl_pair
    gated = gq | gl
    raw = np.abs(at[None, gated, :, :] - sites[:, None, None, :])                           # before the image is taken
    image_margin = float(np.abs(raw - 0.5 * L).min()) if gated.any() else np.inf
    inside = r2[np.broadcast_to(gated[None, :, None], r2.shape)]
    thr = np.array([0.25, 0.5, su["qq_slack"], su["lj_slack"]])
    r_margin = float(np.abs(np.sqrt(inside)[:, None] - np.sqrt(thr)[None, :]).min()) if inside.size else np.inf
    return {"site_lj": site_lj, "A_site_lj": A_lj, "field": field, "A_field": A_field, "phi": phi, "A_phi": A_phi,
            "recip": rec, "A_recip": A_rec, "real": real, "self_phi": self_phi, "site_force": f, "A_site_force": A_f,
            "force": F, "A_force": A_F, "torque": tau, "A_torque": A_tau, "flags": flags, "d": d,
            "image_margin": image_margin, "r_margin": r_margin,
            "pair_min": float(r2[counted].min()) if counted.any() else np.inf, "n_counted": int(counted.sum())}


def fd_safe(ref, step):
    """Whether moving a site by up to `step` keeps every counted pair on its image and on its side of
    r^2 = 0.25, 0.5 and the slacks: what a finite difference of the oracle needs."""
    return ref["image_margin"] > 4 * step and ref["r_margin"] > 4 * step


NAMES = ("force", "torque", "site_lj", "field", "phi", "recip")


def check(su, sol, mol, b, r, out, what="", S=None, ref=None):
    """Every output of replica r in `out` (Batch.solute_forces' dict, or part of it) against replica() on
    the replica's own coordinates and S(k) (S: another S(k) to restate with, e.g. the oracle's of the same
    coordinates).  Returns (the restatement, the worst |x - ref| / A seen)."""
    com, coords, S_own = b.get_replica(r)
    if ref is None:
        ref = replica(su, sol, mol, com, coords, S_own if S is None else S)
    bad, worst = [], 0.0
    assert int(out["flags"][r]) == ref["flags"], (what, r, int(out["flags"][r]), ref["flags"])
    for name in NAMES:
        if name not in out:
            continue
        x = out[name][r]
        if ref["flags"]:
            if np.any(x != 0.0):
                bad.append((name, "not zero in a flagged replica", x.tolist()))
            continue
        A = ref["A_" + name]
        err = np.abs(x - ref[name])
        with np.errstate(all="ignore"):
            worst = max(worst, float(np.nanmax(np.where(A > 0, err / A, 0.0))))
        if not close(x, ref[name], A):
            bad.append((name, x.tolist(), ref[name].tolist(), float((err / (A + 1e-300)).max())))
    assert not bad, f"{what} replica {r}: {bad[:4]}"
    return ref, worst
