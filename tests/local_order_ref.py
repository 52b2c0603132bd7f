"""numpy restatement of mmc_batch_local_order (include/mmc_hip.h, "Local order") for the local-order
tests (not a test module): the four nearest O-O neighbours of every molecule, the tetrahedral order
parameter q of them, and the hydrogen bonds of the Luzar-Chandler geometry, in exactly the
arithmetic the header states -- vector1D images per component, every r^2 and dot product
(x x' + y y') + z z' unfused, ties to the lower index."""
import numpy as np

from structure_ref import vector1d

THIRD = 1.0 / 3.0


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def oo_vectors(coords, box):
    """d[i, j] = d(O_i, O_j) [N, N, 3] and its r^2 [N, N] (coords [3 N, 3]: O, H, H per molecule)."""
    O = np.asarray(coords, dtype=np.float64)[0::3]
    d = vector1d(O[:, None, :], O[None, :, :], box)
    return d, dot3(d, d)


def neighbours(r2):
    """[N, 4]: the four smallest of row i under the key (bits of r2, j), j != i."""
    n = r2.shape[0]
    bits = np.ascontiguousarray(r2).view(np.uint64)
    out = np.empty((n, 4), dtype=np.int32)
    for i in range(n):
        js = np.delete(np.arange(n), i)
        order = np.lexsort((js, bits[i, js]))      # last key first: bits, then j
        out[i] = js[order[:4]]
    return out


def tetrahedral(d, r2, nbr):
    """q_i [N]: 1 - 3/8 sum over (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) of (c_ab + 1/3)^2, in that order;
    NaN where one of the four neighbours is coincident."""
    n = nbr.shape[0]
    q = np.empty(n)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(n):
            dd, rr = d[i, nbr[i]], r2[i, nbr[i]]
            s = None
            for a, b in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
                c = dot3(dd[a], dd[b]) / np.sqrt(rr[a] * rr[b])
                t = (c + THIRD) * (c + THIRD)
                s = t if s is None else s + t
            q[i] = np.nan if np.any(rr == 0.0) else 1.0 - 0.375 * s
    return q


def hbond_matrix(coords, box, r_hb, cos_hb):
    """B[i, h, j] (bool, [N, 2, N]): donor i through its hydrogen h + 1 to acceptor j."""
    c = np.asarray(coords, dtype=np.float64)
    O = c[0::3]
    n = O.shape[0]
    v, r2 = oo_vectors(c, box)
    B = np.zeros((n, 2, n), dtype=bool)
    rhb2, c2 = r_hb * r_hb, cos_hb * cos_hb
    near = r2 < rhb2
    np.fill_diagonal(near, False)
    for h in range(2):
        u = vector1d(O, c[1 + h::3], box)                       # [N, 3]
        t = dot3(u[:, None, :], v)                              # [N, N]
        uu = dot3(u, u)
        B[:, h, :] = near & (t > 0.0) & (t * t >= c2 * (uu[:, None] * r2))
    return B


def q_bin(q, q_bins):
    """The bin of every finite q (int64 [N]; -1 for NaN)."""
    q = np.asarray(q, dtype=np.float64)
    k = np.full(q.shape, -1, dtype=np.int64)
    ok = np.isfinite(q)
    k[ok] = np.minimum(q_bins - 1, np.maximum(0, np.floor((q[ok] + 3.0) * (q_bins / 4.0)).astype(np.int64)))
    return k


def q_histogram(q, q_bins):
    k = q_bin(q, q_bins)
    return np.bincount(k[k >= 0], minlength=q_bins).astype(np.uint64)


def hb_histogram(hb):
    """[3, 9] from hb [N, 2] (donated, accepted, each already clamped to 8)."""
    hb = np.asarray(hb, dtype=np.int64)
    rows = (hb[:, 0], hb[:, 1], np.minimum(hb[:, 0] + hb[:, 1], 8))
    return np.stack([np.bincount(x, minlength=9) for x in rows]).astype(np.uint64)


def local_order(coords, box, r_hb=3.5, cos_hb=np.cos(np.deg2rad(30.0)), q_bins=400):
    """Everything the call returns for one replica: dict with nbr [N, 4] int32, q [N], hb [N, 2]
    uint8, hb_hist [3, 9] uint64, q_hist [q_bins] uint64."""
    d, r2 = oo_vectors(coords, box)
    nbr = neighbours(r2)
    q = tetrahedral(d, r2, nbr)
    B = hbond_matrix(coords, box, r_hb, cos_hb)
    don = np.minimum(B.sum(axis=(1, 2)), 8)
    acc = np.minimum(B.sum(axis=(0, 1)), 8)
    hb = np.stack([don, acc], axis=1).astype(np.uint8)
    return dict(nbr=nbr, q=q, hb=hb, hb_hist=hb_histogram(hb), q_hist=q_histogram(q, q_bins))


# ---- constructed frames for the tests ---------------------------------------------------------------
HOH = np.deg2rad(109.47)   # SPC/E geometry: O-H 1 A, H-O-H 109.47 deg


def water(o, toward, other=None, bond=1.0):
    """O at o, H1 along `toward`, H2 in the plane of `toward` and `other` at the SPC/E angle."""
    o, e1 = np.asarray(o, float), np.asarray(toward, float)
    e1 = e1 / np.linalg.norm(e1)
    t = np.asarray(other if other is not None else ([0.0, 0.0, 1.0] if abs(e1[2]) < 0.9 else [1.0, 0.0, 0.0]), float)
    e2 = t - (t @ e1) * e1
    e2 /= np.linalg.norm(e2)
    return np.array([o, o + bond * e1, o + bond * (np.cos(HOH) * e1 + np.sin(HOH) * e2)])


def frame(oxygens, box, h_dirs=None):
    """[3 N, 3]: a water at every O, its first hydrogen along h_dirs[i] (default +x)."""
    h_dirs = h_dirs or [[1.0, 0.0, 0.0]] * len(oxygens)
    return np.concatenate([water(o, h) for o, h in zip(oxygens, h_dirs)])


def cubic_lattice(n, a):
    g = np.arange(n) * a
    return np.array([[x, y, z] for x in g for y in g for z in g]), n * a
