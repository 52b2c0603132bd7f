"""numpy restatement of mmc_batch_orient_corr for the orientation tests (not a test module): the
definitions of include/mmc_hip.h, "Orientational pair correlations", in unfused fp64.  The image and
the bin are structure_ref.pair_hist's (Ewald/gr.jl:75-91), the axis is the unit vector of
structure_ref.molecule_dipoles."""
import numpy as np

import structure_ref

SCALE = 2.0 ** 30


def axes(com, coords, charge, box):
    """u [N, 3]: mu / sqrt(n^2) with n^2 = (mu_x^2 + mu_y^2) + mu_z^2; 0 where n^2 is 0 or not finite."""
    mu = structure_ref.molecule_dipoles(com, coords, charge, box)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        n2 = (mu[:, 0] * mu[:, 0] + mu[:, 1] * mu[:, 1]) + mu[:, 2] * mu[:, 2]
        ok = np.isfinite(n2) & (n2 > 0.0)
        u = mu / np.sqrt(np.where(ok, n2, 1.0))[:, None]
    return np.where(ok[:, None], u, 0.0)


def quant(v):
    """Q(v): v 2^30 rounded to the nearest integer, ties to even, int64."""
    return np.rint(np.asarray(v, dtype=np.float64) * SCALE).astype(np.int64)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def pair_values(si, ui, sj, uj, side):
    """(r^2, c, hd, p2) of the pairs (i, j) given site 0 and the axis of each side; i one molecule
    or as many as j."""
    sideh = side / 2.0
    d = si - sj
    d = np.where(d < -sideh, d + side, d)
    d = np.where(d > sideh, d - side, d)
    r2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    c = dot3(ui, uj) + np.zeros_like(r2)
    p2 = 1.5 * (c * c) - 0.5
    with np.errstate(invalid="ignore", divide="ignore"):
        hd = np.where(r2 > 0.0, ((3.0 * dot3(ui, d)) * dot3(uj, d)) / r2 - c, 0.0)
    return r2, c, hd, p2


def orient_rows(com, coords, charge, side, numbins, r_max=0.0, reverse=False):
    """int64 [4, numbins + 2] of one frame of 3-site molecules (coords [3 N, 3], com [N, 3]): every
    pair i < j once, bins of r_max / numbins (r_max <= 0: of (side / 2) / numbins), slot
    numbins + 1 for every pair beyond, rows 2 and 3 of that slot 0.  reverse: the pair loop from the
    last pair to the first -- the same sums, being integers."""
    com, coords = np.asarray(com, dtype=np.float64), np.asarray(coords, dtype=np.float64)
    dr = (side / 2.0) / numbins if r_max <= 0 else r_max / numbins
    s0, u = coords[0::3], axes(com, coords, charge, side)
    n = s0.shape[0]
    out = np.zeros((4, numbins + 2), dtype=np.int64)
    order = range(n - 2, -1, -1) if reverse else range(n - 1)
    for i in order:
        js = np.arange(n - 1, i, -1) if reverse else np.arange(i + 1, n)
        r2, c, hd, p2 = pair_values(s0[i], u[i], s0[js], u[js], side)
        b = np.ceil(np.sqrt(r2) / dr)
        b = np.where(b <= numbins, b, numbins + 1).astype(np.int64)
        inr = b <= numbins
        np.add.at(out[0], b, 1)
        np.add.at(out[1], b, quant(c))
        np.add.at(out[2], b[inr], quant(hd[inr]))
        np.add.at(out[3], b[inr], quant(p2[inr]))
    return out
