"""numpy restatement of mmc_batch_pair_energy for the pair-energy tests (not a test module): the
definitions of include/mmc_hip.h, "Pair-energy distributions", in unfused fp64.  The image and the
bin are structure_ref.pair_hist's (Ewald/gr.jl:75-91), the offsets e_a are structure_ref.vector1d's
(Ewald/boundaries.jl), the energy bins are observables.energy_bins'."""
import numpy as np

import structure_ref
from metropolismontecarlo_amd import observables

SCALE = 2.0 ** 20
LIMIT = 2.0 ** 20
NHB = 9


def quant(v):
    """Q(v): v 2^20 rounded to the nearest integer, ties to even, int64."""
    return np.rint(np.asarray(v, dtype=np.float64) * SCALE).astype(np.int64)


def offsets(coords, side):
    """e [N, 3, 3]: e[m, a] = vector1D(site 0 of m, atom a of m); e[:, 0] = 0."""
    coords = np.asarray(coords, dtype=np.float64)
    s0 = coords[0::3]
    return np.stack([structure_ref.vector1d(s0, coords[a::3], side) for a in range(3)], axis=1)


def pair_values(s0i, ei, qi, ti, s0j, ej, qj, tj, eps, sig, factor, side):
    """(r^2, u_C, u_LJ) of the pairs (i, j): i one molecule (s0i [3], ei [3, 3], qi [3], ti [3],
    0-based types), j many (s0j [M, 3], ej [M, 3, 3], qj [M, 3], tj [M, 3])."""
    sideh = side / 2.0
    D = s0i - s0j
    D = np.where(D < -sideh, D + side, D)
    D = np.where(D > sideh, D - side, D)
    r2 = (D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2]
    sc = None
    ulj = np.zeros_like(r2)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for a in range(3):
            P = D + ei[a]
            for b in range(3):
                x = P - ej[:, b]
                r2ab = (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]
                t = (qi[a] * qj[:, b]) / np.sqrt(r2ab)
                sc = t if sc is None else sc + t
                ep, sg = eps[ti[a], tj[:, b]], sig[ti[a], tj[:, b]]
                s2 = (sg * sg) / r2ab
                s6 = (s2 * s2) * s2
                ulj = ulj + np.where(ep > 0.001, (4.0 * ep) * (s6 * s6 - s6), 0.0)
        uc = factor * sc
    return r2, uc, ulj


def direct_sum(coords, atype, charge, eps, sig, factor, side, r_max):
    """(sum u_C, sum u_LJ) in plain fp64 over the pairs i < j with site-0 distance <= r_max."""
    coords = np.asarray(coords, dtype=np.float64)
    s0, e = coords[0::3], offsets(coords, side)
    q, ty = np.asarray(charge, dtype=np.float64).reshape(-1, 3), np.asarray(atype).reshape(-1, 3) - 1
    tc = tl = 0.0
    for i in range(s0.shape[0] - 1):
        js = np.arange(i + 1, s0.shape[0])
        r2, uc, ulj = pair_values(s0[i], e[i], q[i], ty[i], s0[js], e[js], q[js], ty[js], eps, sig, factor, side)
        inr = np.sqrt(r2) <= r_max
        tc += float(uc[inr].sum())
        tl += float(ulj[inr].sum())
    return tc, tl


def pair_energy(coords, atype, charge, eps, sig, factor, side, numbins, r_max=0.0, n_ebins=0, u_lo=0.0, u_hi=1.0,
                u_hb=None, reverse=False):
    """One frame of 3-site molecules (coords [3 N, 3], atype 1-based [3 N], charge [3 N]; eps, sig
    [n_types, n_types]).  Returns a dict: rows int64 [3, numbins + 2]; uhist uint64 [n_ebins + 2]
    (n_ebins > 0); nhb uint64 [9] and cnt int64 [N], the partners below u_hb per molecule (u_hb not
    None); flagged (int); n_below, the pairs with u < u_hb; and `margins`, see margins().  reverse:
    the pair loop from the last pair to the first -- the same sums, being integers."""
    coords = np.asarray(coords, dtype=np.float64)
    eps, sig = np.asarray(eps, dtype=np.float64), np.asarray(sig, dtype=np.float64)
    dr = (side / 2.0) / numbins if r_max <= 0 else r_max / numbins
    s0, e = coords[0::3], offsets(coords, side)
    q, ty = np.asarray(charge, dtype=np.float64).reshape(-1, 3), np.asarray(atype).reshape(-1, 3) - 1
    n = s0.shape[0]
    rows = np.zeros((3, numbins + 2), dtype=np.int64)
    uhist = np.zeros(n_ebins + 2, dtype=np.uint64) if n_ebins > 0 else None
    cnt = np.zeros(n, dtype=np.int64)
    flagged, n_below = 0, 0
    all_u, all_c, all_l = [], [], []
    order = range(n - 2, -1, -1) if reverse else range(n - 1)
    for i in order:
        js = np.arange(n - 1, i, -1) if reverse else np.arange(i + 1, n)
        r2, uc, ulj = pair_values(s0[i], e[i], q[i], ty[i], s0[js], e[js], q[js], ty[js], eps, sig, factor, side)
        b = np.ceil(np.sqrt(r2) / dr)
        b = np.where(b <= numbins, b, numbins + 1).astype(np.int64)
        np.add.at(rows[0], b, 1)
        inr = b <= numbins
        with np.errstate(invalid="ignore"):
            ok = inr & (np.abs(uc) < LIMIT) & (np.abs(ulj) < LIMIT)      # (False for a NaN)
        flagged += int((inr & ~ok).sum())
        np.add.at(rows[1], b[ok], quant(uc[ok]))
        np.add.at(rows[2], b[ok], quant(ulj[ok]))
        u = uc[ok] + ulj[ok]
        if uhist is not None:
            uhist += observables.energy_bins(u, n_ebins, u_lo, u_hi)
        if u_hb is not None:
            below = u < u_hb
            cnt[i] += int(below.sum())
            np.add.at(cnt, js[ok][below], 1)
            n_below += int(below.sum())
        all_u.append(u)
        all_c.append(uc[inr])
        all_l.append(ulj[inr])
    out = dict(rows=rows, uhist=uhist, flagged=flagged, cnt=cnt, n_below=n_below)
    if u_hb is not None:
        out["nhb"] = np.bincount(np.minimum(cnt, NHB - 1), minlength=NHB).astype(np.uint64)
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0)
    out["margins"] = margins(cat(all_u), cat(all_c), cat(all_l), n_ebins, u_lo, u_hi, u_hb)
    return out


def margins(u, uc, ulj, n_ebins, u_lo, u_hi, u_hb):
    """How far the restatement is from every decision the device takes on an energy, in K: a dict of
    `edge`, the unflagged pairs' smallest distance of u to an energy-bin edge; `hb`, of u to u_hb;
    `limit`, the smallest distance of a finite |u_C| or |u_LJ| of a pair in range to the 2^20 flag
    limit.  inf where there is nothing to compare."""
    u = np.asarray(u, dtype=np.float64)
    edge = hb = limit = np.inf
    if n_ebins > 0 and u.size:
        w = (float(u_hi) - float(u_lo)) / n_ebins
        x = (u - u_lo) / w
        inside = np.abs(x - np.rint(x)) * w
        edge = float(np.min(np.where(u < u_lo, u_lo - u, np.where(u > u_hi, u - u_hi, inside))))
    if u_hb is not None and u.size:
        hb = float(np.min(np.abs(u - u_hb)))
    both = np.abs(np.concatenate([np.asarray(uc, dtype=np.float64), np.asarray(ulj, dtype=np.float64)]))
    both = both[np.isfinite(both)]
    if both.size:
        limit = float(np.min(np.abs(both - LIMIT)))
    return dict(edge=edge, hb=hb, limit=limit)
