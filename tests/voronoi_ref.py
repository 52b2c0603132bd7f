"""numpy restatement of mmc_batch_voronoi (include/mmc_hip.h, "Voronoi cells") for the Voronoi tests
(not a test module): every molecule's sorted O-O neighbour list ("Shell order"), one polygon per
neighbour clipped against the other neighbours' half-planes in rising rank, and the cell's volume,
surface, asphericity, faces and flags from them, in exactly the arithmetic the header states --
every dot product (x x' + y y') + z z' unfused, the serial sums as explicit loops in rising rank.
The faces of one molecule are clipped side by side (numpy over the ranks): each element sees the
scalar operations of the header in the header's order.  The polygon is clipped out of place here;
the kernel does it in place, which the header shows to be the same sequence of vertices."""
import functools

import numpy as np

import common
from local_order_ref import cubic_lattice, dot3, frame, oo_vectors
from shell_order_ref import (BOX, SIZES, ball_frame, clamp_bin, coincident_frame, lattice_frame,  # noqa: F401
                             random_frame, replica_frame, water_arrays)

CAP = 64                    # MMC_VORONOI_CAP
MAXV = 16                   # MMC_VORONOI_MAXV
PRUNE = 1.0 + 2.0 ** -20    # MMC_VORONOI_PRUNE
K36PI = 36.0 * 3.141592653589793
F_CAP, F_OPEN, F_POLY = 1, 2, 4
DEFAULTS = dict(r_list=7.0, area_min=0.0, v_bins=200, v_max=80.0, eta_bins=200, eta_max=3.0, r_bins=280)


def params(**kw):
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    return dict(DEFAULTS, **kw)


def qsum(x):
    """k_local_qsum's order over one replica's per-molecule terms (None: left out): lane l adds the
    terms of molecules l, l + 64, ... in that order; the 64 lane sums by an inclusive scan inside
    each row of 16 (steps 1, 2, 4, 8; zero from beyond the row), the four row totals in row order."""
    acc = np.zeros(64)
    for i, v in enumerate(x):
        if v is not None:
            acc[i % 64] = acc[i % 64] + v
    v = acc.reshape(4, 16)
    for s in (1, 2, 4, 8):
        sh = np.zeros_like(v)
        sh[:, s:] = v[:, :-s]
        v = v + sh
    r = v[:, 15]
    return ((r[0] + r[1]) + r[2]) + r[3]


def face_basis(d):
    """(u, v) [n, 3] of the header from the neighbour vectors d [n, 3]."""
    n = len(d)
    ax = np.argmin(np.abs(d), axis=1)                  # the first of equal |components|
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    zero = np.zeros(n)
    w = np.where((ax == 0)[:, None], np.stack([zero, z, -y], 1),
                 np.where((ax == 1)[:, None], np.stack([-z, zero, x], 1), np.stack([y, -x, zero], 1)))
    u = w / np.sqrt(dot3(w, w))[:, None]
    q = np.stack([y * u[:, 2] - z * u[:, 1], z * u[:, 0] - x * u[:, 2], x * u[:, 1] - y * u[:, 0]], 1)
    v = q / np.sqrt(dot3(q, q))[:, None]
    return u, v


def clip_faces(d, r2, r_list, prune=True, stats=None):
    """The n faces of one cell: (S, T [n, MAXV], cnt [n] -- 0: no face --, g [n] the largest
    s s + t t of a face's vertices, poly: a polygon passed MAXV vertices or was cut more than twice)."""
    n = len(r2)
    rl = np.float64(r_list)
    u, v = face_basis(d)
    mk = 0.5 * d
    S, T = np.zeros((n, MAXV)), np.zeros((n, MAXV))
    S[:, :4], T[:, :4] = [-rl, rl, rl, -rl], [-rl, -rl, rl, rl]
    cnt = np.full(n, 4)
    g = np.full(n, rl * rl + rl * rl)
    h = 0.25 * r2
    stopped = np.zeros(n, bool)
    poly = False
    ranks = np.arange(n)
    for m in range(n):
        if prune:
            stopped |= 0.25 * r2[m] > (h + g) * PRUNE
        idx = np.flatnonzero((cnt > 0) & ~stopped & (ranks != m))
        if len(idx) == 0:
            continue
        if stats is not None:
            stats["clips"] = stats.get("clips", 0) + len(idx)
        a, b = dot3(u[idx], d[m]), dot3(v[idx], d[m])
        c = 0.5 * r2[m] - dot3(mk[idx], d[m])
        nv = cnt[idx]
        So, To = S[idx].copy(), T[idx].copy()
        Sn, Tn = np.zeros_like(So), np.zeros_like(To)
        out, cuts = np.zeros(len(idx), int), np.zeros(len(idx), int)
        gn, bad = np.zeros(len(idx)), np.zeros(len(idx), bool)
        rows = np.arange(len(idx))

        def emit(mask, s, t):
            over = mask & (out >= MAXV)
            bad[over] = True
            w = mask & ~over & ~bad
            Sn[rows[w], out[w]], Tn[rows[w], out[w]] = s[w], t[w]
            gn[w] = np.maximum(gn[w], s[w] * s[w] + t[w] * t[w])
            out[w] += 1

        ps, pt = So[:, 0], To[:, 0]
        sp = (a * ps + b * pt) - c
        for j in range(int(nv.max())):
            live = (j < nv) & ~bad
            nxt = np.where(j + 1 < nv, j + 1, 0)
            qs, qt = So[rows, nxt], To[rows, nxt]
            sq = (a * qs + b * qt) - c
            pin, qin = sp <= 0.0, sq <= 0.0
            emit(live & pin, ps, pt)
            cut = live & (pin != qin)
            cuts[cut] += 1
            bad |= cut & (cuts > 2)
            with np.errstate(invalid="ignore", divide="ignore"):
                w = sp / (sp - sq)
                emit(cut & ~bad, ps + w * (qs - ps), pt + w * (qt - pt))
            ps, pt, sp = qs, qt, sq
        if stats is not None:
            stats["max_vertices"] = max(stats.get("max_vertices", 0), int(out[~bad].max(initial=0)))
        poly = poly or bool(bad.any())
        out[bad] = 0
        out[out < 3] = 0
        S[idx], T[idx], cnt[idx], g[idx] = Sn, Tn, out, gn
    return S, T, cnt, g, poly


def face_area(S, T, cnt):
    """A_k = 0.5 |sum of s_j t_(j+1) - s_(j+1) t_j|, the sum from zero in rising j."""
    A = np.zeros(len(cnt))
    for k in range(len(cnt)):
        acc = np.float64(0.0)
        for j in range(cnt[k]):
            jn = j + 1 if j + 1 < cnt[k] else 0
            acc = acc + (S[k, j] * T[k, jn] - S[k, jn] * T[k, j])
        A[k] = 0.5 * abs(acc)
    return A


def cell(d, r2, r_list, area_min=0.0, prune=True, stats=None):
    """One molecule from its sorted list (d [n, 3], r2 [n], n <= CAP): dict with flags, V, S, eta,
    carea, A [n], sides [n], counted [n] (bool)."""
    n = len(r2)
    res = dict(flags=0, V=np.nan, S=np.nan, eta=np.nan, carea=0.0, A=np.zeros(n), sides=np.zeros(n, int),
               counted=np.zeros(n, bool))
    if n == 0 or r2[0] == 0.0:
        res["flags"] = F_OPEN
        return res
    S, T, cnt, g, poly = clip_faces(d, r2, r_list, prune, stats)
    alive = cnt > 0
    rl2 = np.float64(r_list) * np.float64(r_list)
    closed = alive.any() and bool(np.all(4.0 * (0.25 * r2[alive] + g[alive]) <= rl2))
    res["flags"] = (F_POLY if poly else 0) | (0 if closed else F_OPEN)
    if res["flags"]:
        return res
    A = face_area(S, T, cnt)
    rho = np.sqrt(r2)
    counted = A > area_min
    s_sum, t_sum, c_sum = np.float64(0.0), np.float64(0.0), np.float64(0.0)
    for k in range(n):                                           # (a face without area adds 0.0)
        s_sum = s_sum + A[k]
        t_sum = t_sum + A[k] * rho[k]
        c_sum = c_sum + (A[k] if counted[k] else 0.0)
    V = t_sum / 6.0
    with np.errstate(invalid="ignore", divide="ignore"):
        eta = ((s_sum * s_sum) * s_sum) / ((K36PI * V) * V)
    res.update(V=V, S=s_sum, eta=eta, carea=c_sum, A=A, sides=cnt, counted=counted)
    return res


def top_bin(x, bins):
    """(int)floor(x) clamped to 0 .. bins (the slot beyond); bins when x is not finite."""
    return clamp_bin(x, bins) if np.isfinite(x) else bins


def voronoi(coords, box, r_list=7.0, area_min=0.0, v_bins=200, v_max=80.0, eta_bins=200, eta_max=3.0, r_bins=280,
            prune=True, stats=None, mols=None):
    """Everything the call returns for one replica: vol, area [N] (NaN where flagged), faces [N]
    int32, nbr [N, 64] int32, face_area [N, 64], the five histograms (uint64), flagged [3], sums [8];
    and eta [N].  mols: only these molecules (their rows are right; the histograms, flagged and sums
    are then theirs alone, sums in another order than the call's)."""
    box = np.float64(box)
    d, r2 = oo_vectors(coords, box)
    n_mol = r2.shape[0]
    bits = np.ascontiguousarray(r2).view(np.uint64)
    rl2 = np.float64(r_list) * np.float64(r_list)
    v_scale, eta_scale, inv_dr = v_bins / np.float64(v_max), eta_bins / (np.float64(eta_max) - 1.0), r_bins / np.float64(r_list)
    out = dict(vol=np.full(n_mol, np.nan), area=np.full(n_mol, np.nan), faces=np.zeros(n_mol, np.int32),
               nbr=np.full((n_mol, CAP), -1, np.int32), face_area=np.zeros((n_mol, CAP)),
               vol_hist=np.zeros(v_bins + 1, np.uint64), eta_hist=np.zeros(eta_bins + 1, np.uint64),
               face_hist=np.zeros(CAP + 1, np.uint64), side_hist=np.zeros(MAXV + 1, np.uint64),
               nbr_hist=np.zeros(r_bins + 1, np.uint64), flagged=np.zeros(3, np.uint64), sums=np.zeros(8),
               eta=np.full(n_mol, np.nan))
    terms = [[None] * n_mol for _ in range(6)]
    n_ok = 0
    for i in (range(n_mol) if mols is None else mols):
        js = np.flatnonzero(r2[i] < rl2)
        js = js[js != i]
        if len(js) > CAP:
            c = dict(flags=F_CAP)
        else:
            lst = js[np.lexsort((js, bits[i, js]))]                 # last key first: bits, then j
            c = cell(d[i, lst], r2[i, lst], r_list, area_min, prune, stats)
        if c["flags"]:
            out["faces"][i] = -c["flags"]
            for bit in range(3):
                out["flagged"][bit] += (c["flags"] >> bit) & 1
            continue
        k = np.flatnonzero(c["counted"])
        nf = len(k)
        rho = np.sqrt(r2[i, lst])
        out["vol"][i], out["area"][i], out["eta"][i], out["faces"][i] = c["V"], c["S"], c["eta"], nf
        out["nbr"][i, :nf], out["face_area"][i, :nf] = lst[k], c["A"][k]
        out["vol_hist"][top_bin(c["V"] * v_scale, v_bins)] += 1
        out["eta_hist"][top_bin((c["eta"] - 1.0) * eta_scale, eta_bins)] += 1
        out["face_hist"][nf] += 1
        for kk in k:
            out["side_hist"][c["sides"][kk]] += 1
            out["nbr_hist"][top_bin(rho[kk] * inv_dr, r_bins)] += 1
        n_ok += 1
        for q, val in enumerate((c["V"], c["V"] * c["V"], c["S"], c["eta"], np.float64(nf), c["carea"])):
            terms[q][i] = val
    out["sums"][0] = n_ok
    for q in range(6):
        out["sums"][1 + q] = qsum(terms[q])
    return out


def from_details(coords, box, vol, area, faces, nbr, r_list=7.0, area_min=0.0, v_bins=200, v_max=80.0, eta_bins=200,
                 eta_max=3.0, r_bins=280, face_area=None):
    """What follows from a replica's per-molecule outputs by the header's arithmetic: vol_hist,
    eta_hist, face_hist, nbr_hist, flagged and sums (side_hist does not: the sides are not returned)."""
    box = np.float64(box)
    _, r2 = oo_vectors(coords, box)
    v_scale, eta_scale, inv_dr = v_bins / np.float64(v_max), eta_bins / (np.float64(eta_max) - 1.0), r_bins / np.float64(r_list)
    out = dict(vol_hist=np.zeros(v_bins + 1, np.uint64), eta_hist=np.zeros(eta_bins + 1, np.uint64),
               face_hist=np.zeros(CAP + 1, np.uint64), nbr_hist=np.zeros(r_bins + 1, np.uint64),
               flagged=np.zeros(3, np.uint64), sums=np.zeros(8))
    n_mol = len(vol)
    terms = [[None] * n_mol for _ in range(6)]
    for i in range(n_mol):
        if faces[i] < 0:
            for bit in range(3):
                out["flagged"][bit] += (-int(faces[i]) >> bit) & 1
            continue
        V, S = vol[i], area[i]
        with np.errstate(invalid="ignore", divide="ignore"):
            eta = ((S * S) * S) / ((K36PI * V) * V)
        out["vol_hist"][top_bin(V * v_scale, v_bins)] += 1
        out["eta_hist"][top_bin((eta - 1.0) * eta_scale, eta_bins)] += 1
        out["face_hist"][faces[i]] += 1
        c_sum = np.float64(0.0)
        for k in range(faces[i]):
            out["nbr_hist"][top_bin(np.sqrt(r2[i, nbr[i, k]]) * inv_dr, r_bins)] += 1
            if face_area is not None:
                c_sum = c_sum + face_area[i, k]
        out["sums"][0] += 1
        for q, val in enumerate((V, V * V, S, eta, np.float64(faces[i]), c_sum)):
            terms[q][i] = val
    for q in range(6):
        out["sums"][1 + q] = qsum(terms[q])
    return out


# ---- frames ------------------------------------------------------------------------------------------
def basis_lattice(n, a, basis, jitter=0.0, seed=5):
    """n^3 cubic cells of edge a with the given fractional basis: (water arrays, box)."""
    cells, box = cubic_lattice(n, a)
    O = (cells[:, None, :] + a * np.asarray(basis, float)[None, :, :]).reshape(-1, 3)
    if jitter:
        O = O + (np.random.default_rng(seed).random(O.shape) - 0.5) * jitter
    return water_arrays(frame(list(O), box), box)


SC = [[0.0, 0.0, 0.0]]
BCC = [[0.0, 0.0, 0.0], [0.5, 0.5, 0.5]]
FCC = [[0.0, 0.0, 0.0], [0.0, 0.5, 0.5], [0.5, 0.0, 0.5], [0.5, 0.5, 0.0]]
DIAMOND = FCC + [[0.25 + x, 0.25 + y, 0.25 + z] for x, y, z in FCC]
# name: (cells per edge, a, basis, r_list, eta, counted faces at area_min 1e-6, sites per cubic cell)
LATTICES = {
    "sc": (4, 5.5, SC, 9.6, 1.9098593, 6, 1),
    "bcc": (3, 6.0, BCC, 10.4, 1.3273750, 14, 2),
    "fcc": (3, 7.0, FCC, 10.0, 1.3504745, 12, 4),
    "diamond": (2, 10.0, DIAMOND, 9.9, 2.1657437, 16, 8),
}


def lattice(name, jitter=0.0):
    n, a, basis, r_list, eta, faces, per_cell = LATTICES[name]
    return basis_lattice(n, a, basis, jitter), r_list


def nist(k, variant="unwrapped"):
    return common.nist_arrays(k, variant)


@functools.lru_cache(maxsize=None)
def nist_cells(k, variant, r_list, prune=True):
    """(arrays, voronoi() of them, the clip statistics) of a NIST configuration as it stands."""
    a = nist(k, variant)
    stats = {}
    return a, voronoi(a["coords"], a["box"], r_list=r_list, prune=prune, stats=stats), stats


@functools.lru_cache(maxsize=None)
def lattice_cells(name, area_min, jitter=0.0, prune=True):
    a, r_list = lattice(name, jitter)
    return a, voronoi(a["coords"], a["box"], r_list=r_list, area_min=area_min, prune=prune)


RING_R_LIST = 10.0


def ring_frame(k, radius=5.0, gap=2.0):
    """Molecule 0 between two oxygens at +-gap along z, inside a ring of k oxygens at `radius` in its
    own plane: the ring's bisector planes are tangent to one circle, so the two faces towards the
    close pair are regular k-gons and the cell is a closed prism (r_list = RING_R_LIST)."""
    c = np.full(3, 0.5 * BOX)
    phi = 2.0 * np.pi * np.arange(k) / k
    O = [c, c + [0.0, 0.0, gap], c - [0.0, 0.0, gap]] + [c + radius * np.array([np.cos(f), np.sin(f), 0.0]) for f in phi]
    return water_arrays(frame(O, BOX), BOX)
