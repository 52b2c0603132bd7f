"""numpy restatement of mmc_batch_hbond_rings (include/mmc_hip.h, "Hydrogen-bond rings") for the ring
tests (not a test module).  The reference project has no such analysis: the header's definitions are
the specification and this file is their judge.  The graph is network_ref's (bond_matrix, box_vectors) with the donation
matrix from local_order_ref.hbond_matrix; rings_of_graph works straight from the definition: all-pairs
breadth-first distances, every simple cycle up to n_max from its lowest member, the pairwise distance
test, the winding sum and the donation test.  Its `fast` variant walks only the cycles whose members
lie at distance min(k, n - k) from the lowest one (what the kernel searches); the host tests hold the
two against each other.  Also the constructed frames the tests share."""
import numpy as np

from bond_order_ref import TETRA
from local_order_ref import HOH, hbond_matrix
from network_ref import bond_matrix, box_vectors

MAX_SIZE = 8       # MMC_RING_MAX_SIZE
MAX_DEG = 8        # MMC_RING_MAX_DEG
N_STATS = 8        # MMC_RING_STATS
MEMBER_BINS = 33   # MMC_RING_MEMBER_BINS
FAR = 1 << 20


def distances(A, cap):
    """Graph distances int64 [N, N] by breadth-first levels from every molecule at once; FAR where
    there is no path of at most `cap` bonds."""
    n = A.shape[0]
    Af = A.astype(np.float32)
    dist = np.full((n, n), FAR, dtype=np.int64)
    np.fill_diagonal(dist, 0)
    seen = np.eye(n, dtype=bool)
    front = seen.copy()
    for d in range(1, cap + 1):
        front = ((front.astype(np.float32) @ Af) > 0.0) & ~seen
        if not front.any():
            break
        dist[front] = d
        seen |= front
    return dist


def simple_cycles(nbrs, n_max):
    """Every simple cycle of 3 .. n_max members, once: from its lowest member, the smaller of that
    member's two ring neighbours first."""
    for v in range(len(nbrs)):
        path, on = [v], {v}
        stack = [iter(nbrs[v])]
        while stack:
            w = next(stack[-1], None)
            if w is None:
                stack.pop()
                on.discard(path.pop())
                continue
            if w <= v or w in on:
                continue
            path.append(w)
            if len(path) >= 3 and v in nbrs[w] and path[1] < w:
                yield tuple(path)
            if len(path) < n_max:
                on.add(w)
                stack.append(iter(nbrs[w]))
            else:
                path.pop()


def level_cycles(nbrs, dist, n_max):
    """The cycles of simple_cycles whose k-th member is at distance min(k, n - k) from the lowest."""
    for v in range(len(nbrs)):
        lev = dist[v]
        up = [w for w in nbrs[v] if w > v]
        for a in up:
            # (path, descending): ascending members sit at level = index
            todo = [((v, a), False)]
            while todo:
                path, desc = todo.pop()
                x = path[-1]
                lx = int(lev[x])
                for y in nbrs[x]:
                    if y <= v:
                        continue
                    ly = int(lev[y])
                    if not desc:
                        if ly == lx + 1 and 2 * ly <= n_max:
                            todo.append((path + (y,), False))
                            continue
                        if not ((ly == lx and 2 * lx + 1 <= n_max) or (ly == lx - 1 and lx >= 2)):
                            continue
                    elif ly != lx - 1:
                        continue
                    if ly < lx and y == path[ly]:
                        continue
                    if ly == 1:
                        if y > a:
                            yield path + (y,)
                    else:
                        todo.append((path + (y,), True))


def rings_of_graph(A, m, D, n_max=MAX_SIZE, fast=False):
    """The shortest-path rings of the graph A (bool [N, N], symmetric) with box vectors m (int
    [N, N, 3], m[j, i] = -m[i, j]) and donations D (bool [N, N]: i donates to j).  Returns a dict:
    rings = [(members in canonical order, wraps, homodromic)], cycles = the simple cycles looked at."""
    A = np.asarray(A, dtype=bool)
    n = A.shape[0]
    nbrs = [[int(j) for j in np.flatnonzero(A[i])] for i in range(n)]
    dist = distances(A, n_max)
    out, looked = [], 0
    for p in (level_cycles(nbrs, dist, n_max) if fast else simple_cycles(nbrs, n_max)):
        looked += 1
        k = len(p)
        if any(dist[p[a], p[b]] != min(b - a, k - (b - a)) for a in range(k) for b in range(a + 1, k)):
            continue
        nxt = p[1:] + p[:1]
        wind = sum(np.asarray(m[a, b], dtype=np.int64) for a, b in zip(p, nxt))
        homo = all(D[a, b] for a, b in zip(p, nxt)) or all(D[b, a] for a, b in zip(p, nxt))
        wraps = bool(np.any(wind != 0))
        out.append((p, wraps, bool(homo) and not wraps))
    return dict(rings=out, cycles=looked)


def outputs_of_rings(found, n, n_bonds, n_max=MAX_SIZE, max_rings=0):
    """Every output of the call for one unflagged replica from rings_of_graph's list."""
    out = dict(ring_hist=np.zeros((3, MAX_SIZE + 1), dtype=np.uint64),
               member_hist=np.zeros((MAX_SIZE + 1, MEMBER_BINS), dtype=np.uint64),
               stats=np.zeros(N_STATS, dtype=np.int64), count=np.zeros((n, MAX_SIZE + 1), dtype=np.uint16),
               ring=np.full((max_rings, MAX_SIZE), -1, dtype=np.int32))
    cnt = np.zeros((n, MAX_SIZE + 1), dtype=np.int64)
    rows = []
    for p, wraps, homo in found:
        k = len(p)
        out["ring_hist"][1 if wraps else 0, k] += 1
        if wraps:
            continue
        out["ring_hist"][2, k] += int(homo)
        cnt[list(p), k] += 1
        rows.append(p)
    cnt[:, 0] = cnt.sum(1)
    out["count"] = np.minimum(cnt, 65535).astype(np.uint16)
    for k in [0] + list(range(3, n_max + 1)):
        out["member_hist"][k] = np.bincount(np.minimum(cnt[:, k], MEMBER_BINS - 1), minlength=MEMBER_BINS)
    rows.sort()
    for q, p in enumerate(rows[:max_rings]):
        out["ring"][q, :len(p)] = p
    h = out["ring_hist"].astype(np.int64)
    out["stats"][:] = (n_bonds, h[0].sum(), h[1].sum(), h[2].sum(), int((cnt[:, 0] == 0).sum()), cnt[:, 0].max(),
                       max(0, len(rows) - max_rings) if max_rings > 0 else 0, 0)
    out["rows"] = rows
    return out


def graph(coords, box, r_hb, cos_hb):
    """(A, m, D) of one replica under one criterion."""
    return (bond_matrix(coords, box, r_hb, cos_hb), box_vectors(coords, box),
            hbond_matrix(coords, box, r_hb, cos_hb).any(axis=1))


def rings(coords, box, r_hb=3.5, cos_hb=np.cos(np.deg2rad(30.0)), n_max=MAX_SIZE, max_rings=0, fast=True):
    """Everything the call returns for one replica: dict with ring_hist [3, 9] uint64, member_hist
    [9, 33] uint64, stats [8] int64, count [N, 9] uint16, ring [max_rings, 8] int32 (the first rows of
    the sorted list) and, beside them, rows (every row-0 ring, sorted) and A."""
    A, m, D = graph(coords, box, r_hb, cos_hb)
    n = A.shape[0]
    if A.sum(1).max() > MAX_DEG:
        out = outputs_of_rings([], n, 0, n_max, max_rings)
        out["member_hist"][:] = 0
        out["stats"][:] = (0, 0, 0, 0, 0, 0, 0, 1)
        out["count"][:] = 65535
    else:
        out = outputs_of_rings(rings_of_graph(A, m, D, n_max, fast=fast)["rings"], n, int(A.sum()) // 2, n_max, max_rings)
    out["A"] = A
    return out


# ---- hand-made graphs ----------------------------------------------------------------------------------
def graph_of_edges(n, edges):
    """(A, m, D) of a graph that winds nowhere and in which the first of every pair donates."""
    A = np.zeros((n, n), dtype=bool)
    D = np.zeros((n, n), dtype=bool)
    for i, j in edges:
        A[i, j] = A[j, i] = D[i, j] = True
    return A, np.zeros((n, n, 3), dtype=np.int64), D


K4 = (4, [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)])
# two squares 0 1 4 3 and 1 2 5 4 on the grid 0 1 2 / 3 4 5
SQUARES = (6, [(0, 1), (1, 2), (2, 5), (5, 4), (4, 3), (3, 0), (1, 4)])
# corner x + 2 y + 4 z; every corner donates to at most two
CUBE = (8, [(0, 1), (3, 2), (5, 4), (6, 7), (1, 3), (2, 0), (4, 6), (7, 5), (0, 4), (1, 5), (2, 6), (3, 7)])
# hexagon 0 .. 5, centre 6 bonded to the corners 0, 2 and 4
HEX_CENTRE = (7, [(k, (k + 1) % 6) for k in range(6)] + [(6, 0), (6, 2), (4, 6)])
# octagon 0 .. 7 and the bridge 0 - 8 - 9 - 4
OCTAGON = (10, [(k, (k + 1) % 8) for k in range(8)] + [(8, 0), (8, 9), (9, 4)])


# ---- constructed frames --------------------------------------------------------------------------------
def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def donor_frame(O, donations, box, r_hb=3.1, cos_hb=np.cos(np.deg2rad(30.0)), check=True):
    """Waters at the oxygens O (inside the box, no bond across its faces) that realise the directed
    graph `donations` [(donor, acceptor)]: a water that donates twice has both hydrogens in the plane
    of its two acceptors, one beside each; one that donates once has its first hydrogen on the bond
    and the second turned away from its partners; one that donates nothing turns both away.  The
    frame is checked: its bonds and donations under (r_hb, cos_hb) are exactly the ones asked for."""
    O = np.asarray(O, dtype=np.float64)
    n = len(O)
    to = [[] for _ in range(n)]
    partners = [[] for _ in range(n)]
    for i, j in donations:
        to[i].append(j)
        partners[i].append(j)
        partners[j].append(i)
    mols = []
    for i in range(n):
        away = -sum(_unit(O[j] - O[i]) for j in partners[i])
        if np.linalg.norm(away) < 1e-6:
            away = np.array([0.0, 0.0, 1.0])
        if len(to[i]) == 2:
            u, w = _unit(O[to[i][0]] - O[i]), _unit(O[to[i][1]] - O[i])
            mid, side = _unit(u + w), _unit(u - w)
            h = [np.cos(HOH / 2) * mid + np.sin(HOH / 2) * side, np.cos(HOH / 2) * mid - np.sin(HOH / 2) * side]
        elif not to[i]:
            mid = _unit(away)
            d = [_unit(O[j] - O[i]) for j in partners[i]]
            side = np.cross(d[0], d[1]) if len(d) >= 2 else np.cross(mid, [0.3, 0.5, 0.81])
            side = _unit(side - (side @ mid) * mid)
            h = [np.cos(HOH / 2) * mid + np.sin(HOH / 2) * side, np.cos(HOH / 2) * mid - np.sin(HOH / 2) * side]
        else:
            e1 = _unit(O[to[i][0]] - O[i])
            t = away
            e2 = t - (t @ e1) * e1
            e2 = _unit(e2) if np.linalg.norm(e2) > 1e-6 else _unit(np.cross(e1, [0.3, 0.5, 0.81]))
            h = [e1, np.cos(HOH) * e1 + np.sin(HOH) * e2]
        mols.append(np.array([O[i], O[i] + h[0], O[i] + h[1]]))
    coords = np.concatenate(mols)
    A, _, D = graph(coords, box, r_hb, cos_hb)
    want = np.zeros((n, n), dtype=bool)
    for i, j in donations:
        want[i, j] = True
    assert np.all(D[want]) and (not check or (np.array_equal(D, want) and np.array_equal(A, want | want.T))), \
        "the frame does not realise the graph"
    return coords


def polygon(n, box=20.0, pattern=None, bond=2.8):
    """n waters on a planar regular polygon of side `bond` in the middle of the box.  pattern[k]
    says who donates on the bond between k and k + 1: "f" the first, "b" the second, "2" both
    (default: every water donates to the next)."""
    pattern = pattern or "f" * n
    rad = bond / (2.0 * np.sin(np.pi / n))
    O = [np.array([box / 2 + rad * np.cos(2 * np.pi * k / n), box / 2 + rad * np.sin(2 * np.pi * k / n), box / 2])
         for k in range(n)]
    don = []
    for k, c in enumerate(pattern):
        if c in "f2":
            don.append((k, (k + 1) % n))
        if c in "b2":
            don.append(((k + 1) % n, k))
    return donor_frame(O, don, box)


def squares_frame(box=20.0, bond=2.8):
    O = [[box / 2 + bond * (x - 1), box / 2 + bond * (y - 0.5), box / 2] for y in range(2) for x in range(3)]
    return donor_frame(O, SQUARES[1], box)


def cube_frame(box=20.0, bond=2.8):
    O = [[box / 2 + bond * (x - 0.5), box / 2 + bond * (y - 0.5), box / 2 + bond * (z - 0.5)]
         for z in range(2) for y in range(2) for x in range(2)]
    return donor_frame(O, CUBE[1], box)


def octagon_frame(box=20.0, bond=2.8):
    """The octagon in the plane z = L / 2 and, above it, the two waters of the bridge between its
    corners 0 and 4."""
    rad = bond / (2.0 * np.sin(np.pi / 8))
    O = [[box / 2 + rad * np.cos(np.pi * k / 4), box / 2 + rad * np.sin(np.pi * k / 4), box / 2] for k in range(8)]
    z = np.sqrt(bond * bond - (rad - bond / 2) ** 2)
    O += [[box / 2 + bond / 2, box / 2, box / 2 + z], [box / 2 - bond / 2, box / 2, box / 2 + z]]
    return donor_frame(O, OCTAGON[1], box)


def ice_ic(nc, bond=2.75):
    """Proton-ordered cubic ice, nc^3 cells of 8 waters, periodic: the oxygens on
    bond_order_ref.diamond_frame's lattice; one sublattice has its hydrogens along TETRA[0] and
    TETRA[1], the other along -TETRA[2] and -TETRA[3], so every bond carries one hydrogen.  Returns
    (coords, box)."""
    cell = 4.0 * bond / np.sqrt(3.0)
    fcc = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    mols = []
    for i in range(nc):
        for j in range(nc):
            for k in range(nc):
                for sub, shift in ((0, 0.0), (1, 0.25)):
                    for bb in fcc:
                        o = (np.array([i, j, k]) + bb + shift) * cell
                        h = (TETRA[0], TETRA[1]) if sub == 0 else (-TETRA[2], -TETRA[3])
                        mols.append(np.array([o, o + h[0], o + h[1]]))
    return np.concatenate(mols), nc * cell
