"""numpy restatement of mmc_batch_hbond_network (include/mmc_hip.h, "Hydrogen-bond network") for the
network tests (not a test module): the bonds from local_order_ref.hbond_matrix, the degrees, the
sites, the connected components by breadth-first search from the lowest index, the integer offsets
along the search tree and the wrap masks from the edges the tree left out.  Also the constructed
frames the tests share."""
from collections import deque

import numpy as np

from local_order_ref import hbond_matrix, water

MAX_DEG = 16
MAX_CRIT = 8
N_STATS = 8
MAX_MOL = 2048


def bond_matrix(coords, box, r_hb, cos_hb):
    """A[i, j] (bool, symmetric, no diagonal): i donates to j or j to i, through either hydrogen."""
    B = hbond_matrix(coords, box, r_hb, cos_hb).any(axis=1)
    return B | B.T


def box_vectors(coords, box):
    """m[i, j] (int64 [N, N, 3]): the boxes vector1D adds per component to O_j - O_i."""
    O = np.asarray(coords, dtype=np.float64)[0::3]
    d = O[None, :, :] - O[:, None, :]
    m = np.where(np.abs(d) < 0.5 * box, 0.0, -np.copysign(1.0, d))
    return m.astype(np.int64)


def components(A, sites, m):
    """label int32 [N] (-1 off the sites), and per root: size and wrap mask.  Breadth-first from the
    lowest index of every cluster, neighbours in ascending order; p = the sum of m along the tree;
    an edge with p_i + m_ij - p_j != 0 winds."""
    n = A.shape[0]
    label = np.full(n, -1, dtype=np.int32)
    p = np.zeros((n, 3), dtype=np.int64)
    sizes, masks = {}, {}
    for root in range(n):
        if not sites[root] or label[root] >= 0:
            continue
        label[root] = root
        members, queue = [root], deque([root])
        while queue:
            i = queue.popleft()
            for j in np.flatnonzero(A[i] & sites):
                if label[j] < 0:
                    label[j] = root
                    p[j] = p[i] + m[i, j]
                    members.append(j)
                    queue.append(j)
        mask = 0
        for i in members:
            for j in np.flatnonzero(A[i] & sites):
                w = p[i] + m[i, j] - p[j]
                mask |= int(w[0] != 0) | 2 * int(w[1] != 0) | 4 * int(w[2] != 0)
        sizes[root], masks[root] = len(members), mask
    return label, sizes, masks


def network(coords, box, r_hb=3.5, cos_hb=np.cos(np.deg2rad(30.0)), min_bonds=0):
    """Everything the call returns for one replica and one criterion: dict with size_hist [N + 1]
    uint64, deg_hist [17] uint64, stats [8] int64, label [N] int32, nbr [N, 16] int32, and beside
    them masks {root: mask} and sizes {root: size}."""
    A = bond_matrix(coords, box, r_hb, cos_hb)
    n = A.shape[0]
    deg = A.sum(1)
    out = dict(size_hist=np.zeros(n + 1, dtype=np.uint64), deg_hist=np.zeros(MAX_DEG + 1, dtype=np.uint64),
               stats=np.zeros(N_STATS, dtype=np.int64), label=np.full(n, -2, dtype=np.int32),
               nbr=np.full((n, MAX_DEG), -1, dtype=np.int32), masks={}, sizes={}, A=A)
    if deg.max() > MAX_DEG:
        out["stats"][7] = 1
        return out
    out["deg_hist"] = np.bincount(deg, minlength=MAX_DEG + 1).astype(np.uint64)
    for i in range(n):
        js = np.flatnonzero(A[i])
        out["nbr"][i, :len(js)] = js
    sites = deg >= min_bonds
    label, sizes, masks = components(A, sites, box_vectors(coords, box))
    s = np.array(list(sizes.values()), dtype=np.int64)
    out["label"] = label
    out["size_hist"] = np.bincount(s, minlength=n + 1).astype(np.uint64)
    wrapping = [sizes[k] for k in sizes if masks[k]]
    out["stats"][:] = (A.sum() // 2, sites.sum(), len(s), s.max() if len(s) else 0, (s * s).sum(),
                       int(np.bitwise_or.reduce(list(masks.values()))) if masks else 0,
                       max(wrapping) if wrapping else 0, 0)
    out["masks"], out["sizes"] = masks, sizes
    return out


def propagation_rounds(A, sites, label):
    """The largest bond distance of a site from the lowest index of its cluster: the rounds in which
    the kernel's label propagation changes something."""
    n = A.shape[0]
    dist = np.full(n, -1)
    far = 0
    for root in np.flatnonzero(label == np.arange(n)):
        dist[root] = 0
        queue = deque([root])
        while queue:
            i = queue.popleft()
            for j in np.flatnonzero(A[i] & sites):
                if dist[j] < 0:
                    dist[j] = dist[i] + 1
                    far = max(far, dist[j])
                    queue.append(j)
    return far


def brute_force(A, sites, m, bound=3):
    """Clusters and wrap masks with no tree and no potential, straight from the definition: walk the
    covering graph whose nodes are (site, sum of m along the walk so far), sums within +-bound per
    component; a cluster wraps along axis a when its lowest site is reached again with a sum whose
    component a is not zero.  For hand-made graphs.  Returns {frozenset of sites: mask}."""
    n = A.shape[0]
    out, seen_sites = {}, set()
    for start in range(n):
        if not sites[start] or start in seen_sites:
            continue
        seen = {(start, (0, 0, 0))}
        queue = deque(seen)
        while queue:
            i, v = queue.popleft()
            for j in range(n):
                if A[i, j] and sites[j]:
                    w = tuple(int(x) for x in np.array(v) + m[i, j])
                    if max(abs(x) for x in w) <= bound and (j, w) not in seen:
                        seen.add((j, w))
                        queue.append((j, w))
        members = frozenset(i for i, _ in seen)
        mask = 0
        for i, v in seen:
            if i == start:
                mask |= int(v[0] != 0) | 2 * int(v[1] != 0) | 4 * int(v[2] != 0)
        out[members] = mask
        seen_sites |= members
    return out


# ---- constructed frames ------------------------------------------------------------------------------
def torus_line(n, p, box, broken=False):
    """n waters on the closed line O = (0.3, 0.7, L/2) + (t / n) (p L, L, 0), folded into the box;
    every first hydrogen points along (p, 1, 0), so each donates to the next.  broken: molecule 0
    turns its hydrogens away and the ring becomes a path from 1 round to 0."""
    mols = []
    for t in range(n):
        o = (np.array([0.3, 0.7, box / 2]) + (t / n) * np.array([p * box, box, 0.0])) % box
        if broken and t == 0:
            mols.append(water(o, [0.0, 0.0, -1.0], other=[-1.0, float(p), 0.0]))
        else:
            mols.append(water(o, [float(p), 1.0, 0.0]))
    return np.concatenate(mols)


def water_arrays(coords, box):
    """The arrays of a batch of SPC/E-like waters at coords [3 N, 3] (force field of the tests'
    random systems: the call reads coordinates only)."""
    n = len(coords) // 3
    w = np.array([15.9994, 1.008, 1.008])
    com = (coords.reshape(n, 3, 3) * w[None, :, None]).sum(1) / w.sum()
    eps = np.array([[78.2, 0.0], [0.0, 0.0]])
    sig = np.array([[3.166, 1.583], [1.583, 0.0]])
    return dict(com=com, coords=coords, atype=np.tile([1, 2, 2], n).astype(np.int64),
                charge=np.tile([-0.8476, 0.4238, 0.4238], n), eps=eps, sig=sig, box=float(box))


def permuted(coords, perm):
    """Molecule perm[k] of the frame becomes molecule k."""
    return coords.reshape(-1, 3, 3)[perm].reshape(-1, 3)


def translated(coords, shift, box):
    """Every molecule moved by `shift` and carried back into the box by its oxygen."""
    c = coords.reshape(-1, 3, 3) + np.asarray(shift)
    fold = np.floor(c[:, :1, :] / box) * box
    return (c - fold).reshape(-1, 3)
