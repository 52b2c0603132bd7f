"""numpy restatement of mmc_batch_sdf for the spatial-distribution tests (not a test module): the
definitions of include/mmc_hip.h, "Spatial distribution functions", in unfused fp64.  The image is
structure_ref.vector1d (Ewald/boundaries.jl vector1D)."""
import numpy as np

from structure_ref import vector1d


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def frames(coords, box):
    """(s0 [N, 3], axes [N, 3, 3] with rows e_x, e_y, e_z, off [N, 3, 3] with rows o_0 = 0, o_1, o_2,
    ok [N]) of 3-site molecules, coords [3 N, 3]."""
    c = np.asarray(coords, dtype=np.float64)
    s0 = c[0::3]
    o1, o2 = vector1d(s0, c[1::3], box), vector1d(s0, c[2::3], box)
    b, h = o1 + o2, o2 - o1
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        nb2 = dot3(b, b)
        ez = b / np.sqrt(nb2)[:, None]
        t = dot3(h, ez)
        g = h - t[:, None] * ez
        ng2 = dot3(g, g)
        ex = g / np.sqrt(ng2)[:, None]
        ey = np.stack([ez[:, 1] * ex[:, 2] - ez[:, 2] * ex[:, 1],
                       ez[:, 2] * ex[:, 0] - ez[:, 0] * ex[:, 2],
                       ez[:, 0] * ex[:, 1] - ez[:, 1] * ex[:, 0]], axis=1)
    ok = np.isfinite(nb2) & (nb2 > 0.0) & np.isfinite(ng2) & (ng2 > 0.0)
    return s0, np.stack([ex, ey, ez], axis=1), np.stack([np.zeros_like(o1), o1, o2], axis=1), ok


def grid_shape(n_half, fold):
    return (n_half if fold & 1 else 2 * n_half, n_half if fold & 2 else 2 * n_half, 2 * n_half)


def edges(n_half, cell):
    return np.arange(-n_half, n_half + 1).astype(np.float64) * cell


def cell_index(p, n_half, cell, folded):
    """Per coordinate: (index, inside).  e_k <= p < e_k+1 is cell k, stored at k + n_half; a folded
    axis takes |p| and cells 0 .. n_half - 1 stored at k."""
    e = edges(n_half, cell)
    if folded:
        p, e = np.abs(p), e[n_half:]
    with np.errstate(invalid="ignore"):
        k = np.searchsorted(e, p, side="right") - 1       # e[k] <= p < e[k + 1]; a NaN sorts last
        inside = (p >= e[0]) & (p < e[-1])
    return np.where(inside, k, 0), inside


def project(axes, w):
    """p [..., 3]: w on the rows of axes."""
    return np.stack([dot3(axes[..., 0, :], w), dot3(axes[..., 1, :], w), dot3(axes[..., 2, :], w)], axis=-1)


def deposits(coords, box, site_mask):
    """Every deposit of one frame, in the pair loop's order: (centre [M], p [M, 3]) -- for each pair
    i < j and selected slot a, j's site in i's frame and then i's site in j's frame with -d."""
    s0, axes, off, _ = frames(coords, box)
    n = s0.shape[0]
    slots = [a for a in range(3) if site_mask >> a & 1]
    centre, p = [], []
    for i in range(n - 1):
        js = np.arange(i + 1, n)
        d = vector1d(s0[i], s0[js], box)
        for a in slots:
            centre.append(np.full(js.shape, i))
            p.append(project(axes[i], d + off[js, a]))
            centre.append(js)
            p.append(project(axes[js], -d + off[i, a]))
    if not p:
        return np.zeros(0, dtype=np.int64), np.zeros((0, 3))
    return np.concatenate(centre), np.concatenate(p)


def sdf_counts(coords, box, n_half, cell, fold=3, site_mask=1):
    """uint64 [g_x g_y g_z + 2] of one frame: the cells, then outside, then noframe."""
    gx, gy, gz = grid_shape(n_half, fold)
    out = np.zeros(gx * gy * gz + 2, dtype=np.uint64)
    ok = frames(coords, box)[3]
    centre, p = deposits(coords, box, site_mask)
    has = ok[centre]
    out[-1] = np.count_nonzero(~has)
    p = p[has]
    ix, inx = cell_index(p[:, 0], n_half, cell, bool(fold & 1))
    iy, iny = cell_index(p[:, 1], n_half, cell, bool(fold & 2))
    iz, inz = cell_index(p[:, 2], n_half, cell, False)
    inside = inx & iny & inz
    out[-2] = np.count_nonzero(~inside)
    np.add.at(out, ((ix * gy + iy) * gz + iz)[inside], np.uint64(1))
    return out


def on_an_edge(coords, box, n_half, cell, site_mask=7):
    """Whether any projected coordinate of a centre with a frame equals a cell edge (where folding
    on the host and folding in the pass may differ: -e_k is in cell -k, e_k in cell k)."""
    ok = frames(coords, box)[3]
    centre, p = deposits(coords, box, site_mask)
    return bool(np.isin(p[ok[centre]], edges(n_half, cell)).any())


def fold_on_host(grid, fold):
    """A fold = 0 grid [2n, 2n, 2n] folded to `fold`: cell -k - 1 added to cell k."""
    g = np.asarray(grid)
    n = g.shape[0] // 2
    if fold & 1:
        g = g[n:] + g[:n][::-1]
    if fold & 2:
        g = g[:, n:] + g[:, :n][:, ::-1]
    return g
