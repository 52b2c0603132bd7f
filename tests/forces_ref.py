"""Restatement in numpy fp64 of the forces mmc_batch_forces defines (include/mmc_hip.h, "Forces and
torques"), from a replica's (com, coords, S) as Batch.get_replica returns them, and the fixed-order
sums of k_forces_reduce on the host.  Beside each output stands A, the same sum taken over the
absolute values of its terms: the scale the GPU tests' tolerance is a multiple of.  Below them, the
inputs and host-side preconditions of tests/test_gpu_forces_paths.py.  Not a test module."""
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


def check(su, b, r, sel, out, rows, mass=None, what="", refs=None, S=None):
    """Every output of replica r's selected molecules sel (out: Batch.forces' dict with details,
    rows: where molecule sel[k] sits in its arrays) against `molecule` on the replica's own
    coordinates and S(k) (refs: those dicts, where the caller has them already; S: another S(k) to
    restate with in place of get_replica's, e.g. oracle_S of the same coordinates).  Returns the worst
    |x - ref| / A seen (for the record)."""
    com, coords, S_own = b.get_replica(r)
    S = S_own if S is None else S
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


# ---- inputs and preconditions of tests/test_gpu_forces_paths.py (asserted there and, on the starting
# configurations, in tests/test_forces_paths_host.py) ---------------------------------------------
def oracle_S(orc, a, coords, box, alpha=5.6):
    """S(k) of the configuration by the oracle's RecipLong, in the box `box` with kappa = alpha / box:
    what a replica's committed S buffer has to hold (deletion_ref.oracle_terms recomputes it the same
    way)."""
    from metropolismontecarlo_amd import structs
    L = float(box)
    x = np.ascontiguousarray(coords, dtype=np.float64).reshape(-1, 3)
    ew = orc.Ewald(alpha / L, 5, 27, L, factor=structs.factor)
    orc.recip_long(ew, x, np.asarray(a["charge"][:x.shape[0]], dtype=np.float64), L)
    return ew.sumQExpOld.copy()


def com_r2(com, i, box):
    """|vector1D(COM_i, COM_j)|^2 for every j, in molecule()'s arithmetic."""
    com = np.asarray(com, dtype=np.float64)
    rij = vector1D(com[i][None, :], com, box)
    return rij[:, 0] * rij[:, 0] + rij[:, 1] * rij[:, 1] + rij[:, 2] * rij[:, 2]


def between_gates(com, i, lj_rcut, qq_rcut, box):
    """How many other molecules have their COM strictly between the two gates of molecule i: inside
    one and outside the other, so that same_gate == false decides one term of theirs."""
    r2 = com_r2(com, i, box)
    lo, hi = min(lj_rcut, qq_rcut) ** 2, max(lj_rcut, qq_rcut) ** 2
    m = (r2 >= lo) & (r2 < hi)
    m[i] = False
    return int(np.count_nonzero(m))


def first_flush_by(com, i, gate, box):
    """The trip boundary (a multiple of 64 WV_PF) by which the COM scan of unit i has certainly
    emptied its list once, or None: the first one before which more than WV_LIST - 64 WV_PF other
    molecules lie inside the exact gate (common.scan_flushes' lower bound of the prefilter's count).
    No flush can come before the first boundary, 64 WV_PF: a neighbour below that index is in the
    first process() call, one at or above the returned boundary in a later call."""
    import common
    n_list, n_pf = common._wave_list_consts()
    r2 = com_r2(com, i, box)
    gated = r2 < gate * gate * (1 - 1e-9)
    gated[i] = False
    before = np.cumsum(gated)
    for b in range(64 * n_pf, gated.shape[0], 64 * n_pf):
        if before[b - 1] > n_list - 64 * n_pf:
            return b
    return None


def opposite_within(a, mol, r2max=0.5):
    """The molecules other than `mol` with an atom closer than r2max (r^2, minimum image per pair, the
    reference's test is <) to an atom of opposite charge of molecule `mol`, with the smallest such r^2
    each: {molecule: r^2}."""
    x, q, L = np.asarray(a["coords"], dtype=np.float64), np.asarray(a["charge"], dtype=np.float64), float(a["box"])
    out = {}
    for k in range(3 * mol, 3 * mol + 3):
        d = vector1D(x[k][None, :], x, L)
        r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        hit = np.nonzero((r2 < r2max) & (q[:x.shape[0]] * q[k] < 0) & (np.arange(x.shape[0]) // 3 != mol))[0]
        for h in hit:
            out[int(h) // 3] = min(out.get(int(h) // 3, np.inf), float(r2[h]))
    return out


def any_overlap(a):
    """Whether any two molecules of `a` overlap (an opposite-charge atom pair with r^2 < 0.5)."""
    return any(opposite_within(a, m) for m in range(np.asarray(a["com"]).shape[0]))


# test_gpu_deletion.edge_selection's seed for the per-pair-image case with separate cutoffs: the 16
# molecules it gives on config 4 "reference" hold atom pairs between the two slacks, an LJ pair inside
# the LJ gate among them at cutoffs (10, 8) (asserted in tests/test_forces_paths_host.py)
EDGE_SEED = 2

GRID = 2.0 ** -48  # one ulp of a coordinate in [16, 32): every coordinate below 32 A is a multiple of it


def threshold_vector(target, below):
    """A pair vector p on the coordinate grid whose r^2 = (p0 p0 + p1 p1) + p2 p2 is `target` (0.25 or
    0.5) exactly, or with below=True the double just under it, nextafter(target, 0).  Exactly: p =
    (0.5, 0, 0) or (0.5, 0.5, 0), every product and sum exact.  Just under: one component shortened by
    one grid step g and another set to b g, b the integer for which the exact sum of squares,
    target - g + (1 + b^2) g^2, lies nearest the middle of the rounding cell of nextafter(target, 0) --
    within 2^-70 of it where the cell's half width is 2^-56 or 2^-55, so that any order of
    evaluation, fused or not, rounds to that double.  Returns (p [3], u) with u the r^2 intended."""
    from fractions import Fraction
    assert target in (0.25, 0.5)
    p = [0.5, 0.5 if target == 0.5 else 0.0, 0.0]
    if not below:
        return np.array(p), float(target)
    want = float(np.nextafter(target, 0.0))
    g = Fraction(GRID)
    b2 = (g - (Fraction(target) - Fraction(want))) / (g * g) - 1
    b = int(np.sqrt(float(b2)))
    b = min((b - 1, b, b + 1), key=lambda c: abs(c * c - b2))
    free = 2 if target == 0.5 else 1
    short = 1 if target == 0.5 else 0
    p[short] = 0.5 - GRID
    p[free] = b * GRID
    exact = sum(Fraction(c) ** 2 for c in p)
    assert abs(exact - Fraction(want)) < Fraction(2.0 ** -70)
    return np.array(p), want


def r2_unfused(p):
    return (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]


def place_atom(a, mol_i, atom_i, mol_j, atom_j, p):
    """`a` with molecule mol_j translated so that its atom atom_j sits at EXACTLY (atom atom_i of
    mol_i) + p: the sum is checked to be exact in every component, so the difference the kernel and
    the restatement take is p itself, bit for bit.  None where a sum would round (a coordinate
    crossing a power of two) or the pair would need an image."""
    com, x = np.asarray(a["com"], dtype=np.float64).copy(), np.asarray(a["coords"], dtype=np.float64).copy()
    L = float(a["box"])
    xi = x[3 * mol_i + atom_i]
    new = xi + p
    if not (np.array_equal(new - xi, p) and np.all(new > 0.0) and np.all(new < L)):
        return None
    t = new - x[3 * mol_j + atom_j]
    x[3 * mol_j:3 * mol_j + 3] += t
    x[3 * mol_j + atom_j] = new
    com[mol_j] += t
    if not (np.all(com[mol_j] >= 0.0) and np.all(com[mol_j] < L) and np.all(np.abs(com[mol_j] - com[mol_i]) < 0.25 * L)):
        return None
    return dict(a, com=com, coords=x)


def threshold_case(a, target, below, atom_i, mols_i=range(0, 40), mols_j=range(40, 60)):
    """One atom pair of `a` put at r^2 = target exactly, or at the double just under it: the first
    hydrogen of some molecule j against atom atom_i (0: the oxygen, an opposite charge; 1: the first
    hydrogen, a like charge) of some molecule i, the vector one of the signed permutations of
    threshold_vector's.  Taken is the first (i, j, vector) for which the placement is exact and no
    OTHER opposite-charge pair of molecule j lies inside r^2 = 0.7, and no atom pair of j at all
    inside 0.2.  Returns (arrays, i, j, p, u)."""
    import itertools
    p0, u = threshold_vector(target, below)
    x0 = np.asarray(a["coords"], dtype=np.float64)
    L = float(a["box"])
    for i in mols_i:
        if not np.all((x0[3 * i + atom_i] > 4.0) & (x0[3 * i + atom_i] < L - 4.0)):
            continue
        for j in mols_j:
            for perm in sorted(set(itertools.permutations(range(3)))):
                for sg in itertools.product((1.0, -1.0), repeat=3):
                    p = p0[list(perm)] * np.array(sg)
                    c = place_atom(a, i, atom_i, j, 1, p)
                    if c is None:
                        continue
                    near = opposite_within(c, j, 0.7)
                    if atom_i == 0:
                        if set(near) != {i} or sum(1 for _ in _close_pairs(c, j, 0.7, opposite=True)) != 1:
                            continue
                    elif near:
                        continue
                    if any(True for _ in _close_pairs(c, j, 0.2, opposite=None)):
                        continue
                    return c, i, j, p, u
    raise AssertionError("no placement found")


# (target r^2, just under it?, atom of molecule i: 1 a hydrogen -- like charges, the table's first
# node --, 0 the oxygen -- opposite charges, the overlap radius)
THRESHOLDS = ((0.25, False, 1), (0.25, True, 1), (0.5, False, 0), (0.5, True, 0))


def contact_system(a, r2, mols_i=range(0, 40), mols_j=range(40, 60)):
    """volume_perturb_ref.contact_case on `a`: the first hydrogens of two molecules at r^2 = r2 along
    their COM-COM axis, for the first pair (i, j) that leaves no opposite-charge pair of either inside
    r^2 = 0.7 and j's COM in the box.  Returns (arrays, i, j)."""
    import volume_perturb_ref as vp
    L = float(a["box"])
    for i in mols_i:
        for j in mols_j:
            c, _ = vp.contact_case(a, i, j, r2)
            if np.all((c["com"][j] >= 0) & (c["com"][j] < L)) and not opposite_within(c, j, 0.7) \
                    and not opposite_within(c, i, 0.7):
                return c, i, j
    raise AssertionError("no contact found")


def _close_pairs(a, mol, r2max, opposite):
    """(atom of mol, other atom, r^2) of the atom pairs of molecule `mol` with r^2 < r2max; opposite:
    True for opposite charges only, None for every pair."""
    x, q, L = np.asarray(a["coords"], dtype=np.float64), np.asarray(a["charge"], dtype=np.float64), float(a["box"])
    for k in range(3 * mol, 3 * mol + 3):
        d = vector1D(x[k][None, :], x, L)
        r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        m = (r2 < r2max) & (np.arange(x.shape[0]) // 3 != mol)
        if opposite:
            m &= q[:x.shape[0]] * q[k] < 0
        for h in np.nonzero(m)[0]:
            yield k, int(h), float(r2[h])


def pair_r2(a, mol_i, atom_i, mol_j, atom_j):
    """r^2 of one atom pair in molecule()'s arithmetic (vector1D, the unfused sum)."""
    x = np.asarray(a["coords"], dtype=np.float64)
    p = vector1D(x[3 * mol_i + atom_i], x[3 * mol_j + atom_j], float(a["box"]))
    return float(r2_unfused(p))


def slack_pairs(su, com, coords, sel):
    """The atom pairs of the selected molecules that the two slacks treat differently: inside a COM
    gate with r^2 (per-pair image) at or above the smaller slack and below the larger.  Returns
    (all such pairs inside either gate, the LJ pairs among them inside the LJ gate -- where `lon`
    tested against the wrong slack would change w_lj and the forces --, the charged pairs among them
    inside the Coulomb gate)."""
    com, at = np.asarray(com, dtype=np.float64), np.asarray(coords, dtype=np.float64).reshape(-1, 3, 3)
    lo, hi = min(su["lj_slack"], su["qq_slack"]), max(su["lj_slack"], su["qq_slack"])
    n_all = n_lj = n_qq = 0
    qq = su["q"][:, None] * su["q"][None, :]
    for i in sel:
        c = com_r2(com, int(i), su["box"])
        others = np.arange(com.shape[0]) != i
        gq, gl = others & (c < su["qq_gate"]), others & (c < su["lj_gate"])
        rab = vector1D(at[int(i)][None, :, None, :], at[:, None, :, :], su["box"])
        r2 = rab[..., 0] * rab[..., 0] + rab[..., 1] * rab[..., 1] + rab[..., 2] * rab[..., 2]
        mid = (r2 >= lo) & (r2 < hi)
        n_all += int(np.count_nonzero(mid & (gq | gl)[:, None, None]))
        n_lj += int(np.count_nonzero(mid & gl[:, None, None] & (su["eps"][None] > 0.001)))
        n_qq += int(np.count_nonzero(mid & gq[:, None, None] & (qq[None] != 0)))
    return n_all, n_lj, n_qq


def shifted_replica(a, k):
    """Replica k's configuration of the small-system cases: `a` translated rigidly by a vector of
    its own and wrapped molecule by molecule (by COM) into the box."""
    L = float(a["box"])
    shift = np.array([1.3 + 0.7 * k, -2.1 + 0.4 * k, 0.4 - 0.9 * k]) * (k > 0)
    com0 = np.asarray(a["com"], dtype=np.float64)
    com = (com0 + shift) % L
    return com, np.asarray(a["coords"], dtype=np.float64) + np.repeat(com - com0, 3, axis=0)


def flush_system():
    """The system of test_gpu_deletion_paths.py::test_neighbour_list_flush -- 2000 SPC/E molecules at
    0.06 / A^3 with 12.4 A cutoffs -- and 24 molecules whose scan certainly empties its list mid-way
    (common.scan_flushes).  Returns (arrays, r_cut, sel)."""
    import common
    from test_gpu_batch import _dense_water
    a = _dense_water(2000, rho=0.06)
    L, rc = float(a["box"]), 12.4
    com = np.asarray(a["com"])
    rng = np.random.default_rng(2000)
    sel = [int(i) for i in rng.permutation(2000) if common.scan_flushes(com, [com[i]], rc, L, exclude=int(i))][:24]
    return a, rc, np.array(sel)


def flush_overlap(a, rc):
    """flush_system's arrays with one opposite-charge overlap planted (volume_perturb_ref.overlap_case,
    r^2 = 0.3) between a molecule i < 64 WV_PF and a molecule j at or beyond the boundary by which unit
    i has flushed: unit i meets j after its first flush, unit j meets i in its first process() call and
    flushes afterwards.  Taken is the first (i, j) for which these hold IN THE PLANTED SYSTEM, both
    scans flush, and no third molecule overlaps either.  Returns (arrays, i, j)."""
    import common
    import volume_perturb_ref as vp
    L = float(a["box"])
    com = np.asarray(a["com"])
    n = com.shape[0]
    trip = 64 * common._wave_list_consts()[1]
    for i in range(0, trip):
        bi = first_flush_by(com, i, rc, L)
        if bi is None:
            continue
        for j in range(n - 1, bi + 64, -1):
            c, _ = vp.overlap_case(a, i, j, r2=0.3)
            if not np.all((c["com"][j] >= 0) & (c["com"][j] < L)):
                continue
            if flush_overlap_ok(c, rc, i, j):
                return c, i, j
    raise AssertionError("no pair found")


def flush_overlap_ok(c, rc, i, j):
    """flush_overlap's conditions on the planted system c."""
    import common
    L, com = float(c["box"]), np.asarray(c["com"])
    trip = 64 * common._wave_list_consts()[1]
    bi = first_flush_by(com, i, rc, L)
    return (i < trip and bi is not None and j >= bi and com_r2(com, i, L)[j] < rc * rc * (1 - 1e-9)
            and common.scan_flushes(com, [com[i]], rc, L, exclude=i)
            and common.scan_flushes(com, [com[j]], rc, L, exclude=j)
            and set(opposite_within(c, j)) == {i} and set(opposite_within(c, i)) == {j})
