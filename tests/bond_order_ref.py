"""numpy restatement of mmc_batch_bond_order (include/mmc_hip.h, "Bond order") for the bond-order
tests (not a test module): every molecule's O-O neighbours inside r_nb sorted under (bits of r^2, j),
the harmonics of the nearest n_nb bonds by the header's recurrences, q_lm, Q, q_l, the bond
correlations, the windows, qbar_l, the solid-like molecules and their clusters -- in exactly the
arithmetic the header states: every operation a separate correctly rounded fp64 one, the serial sums
as explicit loops in rank order and in rising m -- and the frames that the CPU and the GPU tests
share.  legendre_q and legendre_c are the independent form: the addition theorem over Legendre
polynomials of the bond angles, with no spherical harmonics in it."""
import numpy as np

from local_order_ref import frame, oo_vectors
from shell_order_ref import BOX, clamp_bin, water_arrays
from structure_ref import vector1d

CAP = 64        # MMC_SHELL_CAP
NBR = 16        # MMC_BO_MAX_NB
PI = np.float64(3.141592653589793)
INF = float("inf")
DEFAULTS = dict(l=3, r_nb=3.5, n_nb=4, a=(-INF, -0.8), b=(-0.35, 0.25), min_a=3, min_ab=4, q_bins=200, c_bins=200)
HISTS = ("q_hist", "qbar_hist", "c_hist", "ab_hist", "size_hist")
DETAILS = ("q", "qbar", "nbr", "ab", "label")


def params(**kw):
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    return dict(DEFAULTS, **kw)


def constants(l):
    """N_m [l + 1] and K of the header."""
    norm = []
    for m in range(l + 1):
        F = np.float64(1.0)
        for k in range(l - m + 1, l + m + 1):
            F = F * np.float64(k)
        norm.append(np.sqrt((np.float64(2 * l + 1) / (np.float64(4.0) * PI)) / F))
    return norm, (np.float64(4.0) * PI) / np.float64(2 * l + 1)


def harmonics(x, y, z, l):
    """Re Y_lm and Im Y_lm, m = 0 .. l (two lists of arrays shaped like x), by the header's recurrences."""
    norm, _ = constants(l)
    c, s, tmm = np.ones_like(x), np.zeros_like(x), np.float64(1.0)
    re, im = [], []
    for m in range(l + 1):
        if m > 0:
            c, s = x * c - y * s, x * s + y * c
            tmm = tmm * np.float64(2 * m - 1)
        t = np.full_like(x, tmm)
        if m < l:
            t2 = t
            t = (np.float64(2 * m + 1) * z) * tmm
            for n in range(m + 2, l + 1):
                t, t2 = (((np.float64(2 * n - 1) * z) * t) - (np.float64(n + m - 1) * t2)) / np.float64(n - m), t
        A = norm[m] * t
        re.append(A * c)
        im.append(A * s)
    return re, im


def rank_sum(first, terms, n):
    """first + terms[:, 0] + terms[:, 1] + ..., one at a time, row i taking its first n[i] terms
    (first None: the sum starts with terms[:, 0])."""
    acc = terms[:, 0].copy() if first is None else first.copy()
    for k in range(0 if first is not None else 1, terms.shape[1]):
        acc = np.where(k < n, acc + terms[:, k], acc)
    return acc


def norm2(re, im):
    """Q of the header from [l + 1, ...] real and imaginary parts: t_0 + 2 t_1 + ... in rising m."""
    Q = re[0] * re[0] + im[0] * im[0]
    for m in range(1, len(re)):
        Q = Q + np.float64(2.0) * (re[m] * re[m] + im[m] * im[m])
    return Q


def neighbour_lists(coords, box, r_nb, n_nb):
    """nbr [N, 16] int32 (-1 beyond n_i), n [N], count [N] (-1 where flagged), d [N, N, 3], r2 [N, N]."""
    d, r2 = oo_vectors(coords, np.float64(box))
    n_mol = r2.shape[0]
    bits = np.ascontiguousarray(r2).view(np.uint64)
    rnb2 = np.float64(r_nb) * np.float64(r_nb)
    nbr = np.full((n_mol, NBR), -1, np.int32)
    n, count = np.zeros(n_mol, np.int64), np.zeros(n_mol, np.int64)
    for i in range(n_mol):
        js = np.flatnonzero(r2[i] < rnb2)
        js = js[js != i]
        if len(js) > CAP:
            count[i] = -1
            continue
        lst = js[np.lexsort((js, bits[i, js]))]
        count[i] = len(js)
        n[i] = min(len(js), n_nb)
        nbr[i, :n[i]] = lst[:n[i]]
    return nbr, n, count, d, r2


def clusters(solid, nbr):
    """label [N] int32: the lowest index of the connected component of every solid-like molecule
    under the edges {i, j}, j in nb(i), both solid-like; -1 elsewhere."""
    n_mol = len(solid)
    parent = np.arange(n_mol)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i in np.flatnonzero(solid):
        for j in nbr[i]:
            if j >= 0 and solid[j]:
                a, b = find(i), find(j)
                parent[max(a, b)] = min(a, b)
    return np.array([find(i) if solid[i] else -1 for i in range(n_mol)], np.int32)


def bond_order(coords, box, l=3, r_nb=3.5, n_nb=4, a=(-INF, -0.8), b=(-0.35, 0.25), min_a=3, min_ab=4, q_bins=200,
               c_bins=200):
    """Everything the call returns for one replica, under the names of Batch.bond_order (stats [8],
    no sums), and c [N, 16] (NaN where the bond is undefined or absent), defined, flagged [N] bool."""
    nbr, n, count, d, r2 = neighbour_lists(coords, box, r_nb, n_nb)
    n_mol = len(n)
    _, K = constants(l)
    flagged = count < 0
    k16 = np.arange(NBR)[None, :]
    used = k16 < n[:, None]
    jj = np.where(used, nbr, 0)
    rows = np.arange(n_mol)[:, None]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rr = np.where(used, r2[rows, jj], 1.0)
        rho = np.sqrt(rr)
        undefined = ~flagged & ((n == 0) | np.any(used & (rr == 0.0), axis=1))
        defined = ~flagged & ~undefined
        dd = d[rows, jj]
        re, im = harmonics(dd[..., 0] / rho, dd[..., 1] / rho, dd[..., 2] / rho, l)
        nn = np.maximum(n, 1).astype(np.float64)
        qre = [rank_sum(None, t, n) / nn for t in re]                       # [l + 1][N]
        qim = [rank_sum(None, t, n) / nn for t in im]
        Q = norm2(qre, qim)
        q = np.where(defined, np.sqrt(K * Q), np.nan)
        # bonds
        D = None
        for m in range(l + 1):
            t = qre[m][:, None] * qre[m][jj] + qim[m][:, None] * qim[m][jj]
            D = t if m == 0 else D + np.float64(2.0) * t
        c = D / (np.sqrt(Q)[:, None] * np.sqrt(Q[jj]))
        bond = used & defined[:, None] & defined[jj] & (Q[:, None] != 0.0) & (Q[jj] != 0.0) & np.isfinite(c)
        in_a = bond & (c >= np.float64(a[0])) & (c <= np.float64(a[1]))
        in_b = bond & (c >= np.float64(b[0])) & (c <= np.float64(b[1]))
        n_a, n_b = in_a.sum(1), in_b.sum(1)
        solid = defined & (n_a >= min_a) & (n_a + n_b >= min_ab)
        # averaged
        def_bar = defined & ~np.any(used & ~defined[jj], axis=1)
        bre = [rank_sum(qre[m], qre[m][jj], n) / (n + 1).astype(np.float64) for m in range(l + 1)]
        bim = [rank_sum(qim[m], qim[m][jj], n) / (n + 1).astype(np.float64) for m in range(l + 1)]
        qbar = np.where(def_bar, np.sqrt(K * norm2(bre, bim)), np.nan)
    label = clusters(solid, nbr)
    roots, sizes = np.unique(label[label >= 0], return_counts=True)

    out = dict(q=q, qbar=qbar, nbr=nbr, ab=np.stack([n_a, n_b], axis=1).astype(np.uint8), label=label,
               c=np.where(bond, c, np.nan), defined=defined, flagged=flagged, used=used, n=n,
               q_hist=np.zeros(q_bins + 1, np.uint64), qbar_hist=np.zeros(q_bins + 1, np.uint64),
               c_hist=np.zeros(c_bins + 1, np.uint64), ab_hist=np.zeros((17, 17), np.uint64),
               size_hist=np.bincount(sizes, minlength=n_mol + 1).astype(np.uint64))
    for i in range(n_mol):
        out["q_hist"][clamp_bin(q[i] * np.float64(q_bins), q_bins - 1) if defined[i] else q_bins] += 1
        out["qbar_hist"][clamp_bin(qbar[i] * np.float64(q_bins), q_bins - 1) if def_bar[i] else q_bins] += 1
        if defined[i]:
            out["ab_hist"][n_a[i], n_b[i]] += 1
        for k in range(n[i]):
            out["c_hist"][clamp_bin((c[i, k] + 1.0) * (c_bins / 2.0), c_bins - 1) if bond[i, k] else c_bins] += 1
    out["stats"] = np.array([defined.sum(), undefined.sum(), flagged.sum(), np.count_nonzero(count > n_nb), solid.sum(),
                             len(sizes), sizes.max() if len(sizes) else 0, (sizes.astype(np.int64) ** 2).sum()], np.int64)
    return out


# ---- the independent form: Legendre polynomials of the bond angles ----------------------------------
def unit_bonds(coords, box, nbr, i):
    O = np.asarray(coords, dtype=np.float64)[0::3]
    js = nbr[i][nbr[i] >= 0]
    d = vector1d(O[i][None, :], O[js], np.float64(box))
    return d / np.sqrt((d * d).sum(1))[:, None]


def legendre(l, x):
    return np.polynomial.legendre.legval(x, [0.0] * l + [1.0])


def legendre_q(coords, box, nbr, i, l):
    """q_l(i) = sqrt(sum over j, k in nb(i) of P_l(u_ij . u_ik)) / n_i."""
    u = unit_bonds(coords, box, nbr, i)
    return np.sqrt(max(legendre(l, np.clip(u @ u.T, -1.0, 1.0)).sum(), 0.0)) / len(u)


def legendre_c(coords, box, nbr, i, j, l):
    """c_ij = sum over k in nb(i), k' in nb(j) of P_l(u_ik . u_jk') / (n_i n_j q_l(i) q_l(j))."""
    u, v = unit_bonds(coords, box, nbr, i), unit_bonds(coords, box, nbr, j)
    s = legendre(l, np.clip(u @ v.T, -1.0, 1.0)).sum() / (len(u) * len(v))
    return s / (legendre_q(coords, box, nbr, i, l) * legendre_q(coords, box, nbr, j, l))


# ---- frames for the tests: each returns the arrays of a batch (tests/common.py) ---------------------
SIZES = (2, 3, 64, 65, 66, 129)
TETRA = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) / np.sqrt(3.0)


def oxygen_frame(O, box):
    """Waters (first hydrogen along +x) at the given oxygens."""
    return water_arrays(frame([list(p) for p in np.asarray(O, float)], box), box)


def sc_frame(spacing=7.4):
    """Simple cubic, 3^3 sites, periodic: six neighbours at `spacing`, twelve at spacing sqrt(2)."""
    g = np.arange(3) * spacing
    return oxygen_frame([[x, y, z] for x in g for y in g for z in g], 3 * spacing), 1.2 * spacing


def fcc_frame(cell=11.0):
    """fcc, 2^3 cells, 32 sites, periodic: twelve neighbours at cell / sqrt(2), six at cell."""
    basis = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    O = [(np.array([i, j, k]) + bb) * cell for i in range(2) for j in range(2) for k in range(2) for bb in basis]
    return oxygen_frame(O, 2 * cell), 0.85 * cell


def diamond_frame(cell=11.0):
    """Cubic diamond (the oxygens of ice Ic), 2^3 cells, 64 sites, periodic: four neighbours at
    cell sqrt(3) / 4, twelve at cell / sqrt(2)."""
    fcc = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    basis = np.concatenate([fcc, fcc + 0.25])
    O = [(np.array([i, j, k]) + bb) * cell for i in range(2) for j in range(2) for k in range(2) for bb in basis]
    return oxygen_frame(O, 2 * cell), 0.55 * cell


def wurtzite_fragment(bond=2.75):
    """17 oxygens of hexagonal ice around molecule 0, not periodic: its four neighbours (1 .. 4) on a
    tetrahedron and their three further neighbours each (5 .. 16).  The bond to neighbour 1 is
    eclipsed -- the far end's bonds are the mirror images of the centre's in the plane across the
    bond -- the other three staggered: the far end's bonds are the inversions of the centre's."""
    c = np.full(3, 0.5 * BOX)
    O = [c] + [c + bond * t for t in TETRA]
    for k in range(4):
        for j in range(4):
            if j == k:
                continue
            if k == 0:
                e = TETRA[j] - 2.0 * (TETRA[j] @ TETRA[0]) * TETRA[0]
            else:
                e = -TETRA[j]
            O.append(c + bond * TETRA[k] + bond * e)
    return oxygen_frame(O, BOX)


LINE_N, LINE_STEP = 128, 3.0


def line_frame():
    """128 oxygens 3 A apart on a line along x, index 0 at one end, in a box that keeps the ends apart."""
    box = LINE_N * LINE_STEP + 16.0
    O = [[8.0 + LINE_STEP * k, 0.5 * box, 0.5 * box] for k in range(LINE_N)]
    return oxygen_frame(O, box)


def bridging_frame():
    """Two rows of six oxygens along x with gaps 2.6, 2.7, 2.8, 2.9, 3.0: with n_nb = 1 every molecule
    lists the one before it in its row (the first lists the second), so the edges beyond the first are
    listed from one end only.  Row one is indexed in rising x (the lister has the higher index: it
    pulls the label), row two in falling x (the lister has the lower index: it pushes)."""
    x = np.concatenate([[0.0], np.cumsum([2.6, 2.7, 2.8, 2.9, 3.0])])
    row1 = [[4.0 + v, 6.0, 11.0] for v in x]
    row2 = [[4.0 + v, 16.0, 11.0] for v in x[::-1]]
    return oxygen_frame(row1 + row2, BOX)


def rotation(seed):
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else q[:, ::-1]
