"""CPU tests of the hydrogen-bond network's host side: the numpy restatement (tests/network_ref.py)
against a brute-force search that uses no spanning tree, on hand-made graphs and on the torus lines
the GPU tests run, and the observables on hand-made histograms."""
import numpy as np
import pytest

import common
import network_ref as ref
from local_order_ref import water
from metropolismontecarlo_amd import observables as obs

COS30 = float(np.cos(np.deg2rad(30.0)))


def check_against_brute_force(A, sites, m, bound=3):
    label, sizes, masks = ref.components(A, sites, m)
    brute = ref.brute_force(A, sites, m, bound)
    assert {frozenset(np.flatnonzero(label == root)): masks[root] for root in sizes} == brute
    assert all(label[i] == min(c) for c in brute for i in c)
    assert np.all(label[~sites] == -1)
    return label, sizes, masks


def graph(n, edges):
    """A and m of a hand-made graph: edges (i, j, (mx, my, mz)) with m_ji = -m_ij."""
    A, m = np.zeros((n, n), dtype=bool), np.zeros((n, n, 3), dtype=np.int64)
    for i, j, v in edges:
        A[i, j] = A[j, i] = True
        m[i, j], m[j, i] = v, -np.asarray(v)
    return A, m


def test_two_triangles_and_a_loner():
    """One triangle inside the box, one whose three edges each cross a face but sum to zero, one
    that winds along y; site 6 has no edges."""
    A, m = graph(10, [(0, 1, (0, 0, 0)), (1, 2, (0, 0, 0)), (0, 2, (0, 0, 0)),
                      (3, 4, (1, 0, 0)), (4, 5, (-1, 0, 0)), (3, 5, (0, 0, 0)),
                      (7, 8, (0, 1, 0)), (8, 9, (0, 0, 0)), (7, 9, (0, 0, 0))])
    sites = np.ones(10, dtype=bool)
    label, sizes, masks = check_against_brute_force(A, sites, m)
    assert list(label) == [0, 0, 0, 3, 3, 3, 6, 7, 7, 7]
    assert sizes == {0: 3, 3: 3, 6: 1, 7: 3} and masks == {0: 0, 3: 0, 6: 0, 7: 2}
    # the selection cuts the graph: without site 8 the winding triangle is a path
    sites[8] = False
    label, sizes, masks = check_against_brute_force(A, sites, m)
    assert label[8] == -1 and sizes[7] == 2 and masks[7] == 0


def test_a_gauge_change_moves_no_mask():
    """Storing a molecule one box over adds the same vector to m on all its edges."""
    A, m = graph(4, [(0, 1, (0, 0, 0)), (1, 2, (0, 0, 1)), (2, 3, (0, 0, 0)), (0, 3, (0, 0, 0))])
    sites = np.ones(4, dtype=bool)
    _, _, masks = check_against_brute_force(A, sites, m)
    assert masks == {0: 4}
    g = np.array([1, -1, 0])
    m2 = m.copy()
    for j in np.flatnonzero(A[2]):
        m2[2, j] += g
        m2[j, 2] -= g
    _, _, masks2 = check_against_brute_force(A, sites, m2, bound=4)
    assert masks2 == masks


def ring_across_a_face(box=20.0, n=7):
    """n waters in a row along x, 20 / 7 = 2.857 A apart, every first hydrogen along +x: a ring that
    closes through the face x = L."""
    return np.concatenate([water([0.2 + t * box / n, 5.0, 5.0], [1.0, 0.0, 0.0]) for t in range(n)]), box


def test_ring_across_a_face():
    coords, box = ring_across_a_face()
    w = ref.network(coords, box, 3.5, COS30)
    assert list(w["stats"]) == [7, 7, 1, 7, 49, 1, 7, 0]
    assert np.all(w["label"] == 0) and w["size_hist"][7] == 1 and w["deg_hist"][2] == 7
    A = w["A"]
    check_against_brute_force(A, np.ones(7, dtype=bool), ref.box_vectors(coords, box))
    # min_bonds above the degree: no sites at all
    w = ref.network(coords, box, 3.5, COS30, min_bonds=3)
    assert list(w["stats"]) == [7, 0, 0, 0, 0, 0, 0, 0] and np.all(w["label"] == -1) and w["size_hist"].sum() == 0
    # a narrow cone keeps the bonds (the hydrogens point straight at the acceptors), a short r_hb none
    assert ref.network(coords, box, 3.5, 1.0)["stats"][0] == 7
    assert ref.network(coords, box, 2.8, COS30)["stats"][2] == 7


@pytest.mark.parametrize("n,p,box", [(129, 8, 44.8), (65, 4, 45.3)])
def test_torus_lines(n, p, box):
    """The closed line winds p times along x and once along y; with molecule 0 turned away it is a
    path of n - 1 bonds whose lowest index sits at one end."""
    for broken in (False, True):
        coords = ref.torus_line(n, p, box, broken)
        w = ref.network(coords, box, 3.5, COS30)
        bonds, mask = (n - 1, 0) if broken else (n, 3)
        assert list(w["stats"]) == [bonds, n, 1, n, n * n, mask, n if mask else 0, 0], (broken, w["stats"])
        sites = np.ones(n, dtype=bool)
        check_against_brute_force(w["A"], sites, ref.box_vectors(coords, box), bound=p + 1)
        rounds = ref.propagation_rounds(w["A"], sites, w["label"])
        assert rounds == (n - 1 if broken else n // 2)
        # sizes and masks survive a relabelling and a rigid translation; labels follow the permutation
        rng = np.random.default_rng(n + broken)
        perm = rng.permutation(n)
        wp = ref.network(ref.permuted(coords, perm), box, 3.5, COS30)
        assert np.array_equal(wp["stats"], w["stats"]) and np.all(wp["label"] == 0)
        wt = ref.network(ref.translated(coords, rng.random(3) * box, box), box, 3.5, COS30)
        assert np.array_equal(wt["stats"], w["stats"]) and np.array_equal(wt["nbr"], w["nbr"])


def test_flagged_frames_have_the_defined_values():
    a = common.nist_arrays(1, "unwrapped")
    w = ref.network(a["coords"], a["box"], 7.0, float(np.cos(np.deg2rad(75.0))))
    n = len(a["coords"]) // 3
    assert w["A"].sum(1).max() > ref.MAX_DEG
    assert list(w["stats"]) == [0] * 7 + [1] and np.all(w["label"] == -2) and np.all(w["nbr"] == -1)
    assert w["size_hist"].shape == (n + 1,) and w["size_hist"].sum() == 0 and w["deg_hist"].sum() == 0


def test_nist_configuration_4_percolates_at_3p5_and_not_at_3p0():
    a = common.nist_arrays(4, "unwrapped")
    w = ref.network(a["coords"], a["box"], 3.5, COS30)
    assert w["stats"][5] == 7 and w["stats"][6] == w["stats"][3] > 600
    assert w["stats"][1] == 750 and w["size_hist"] @ np.arange(751) == 750
    w3 = ref.network(a["coords"], a["box"], 3.0, COS30)
    assert w3["stats"][5] == 0 and w3["stats"][6] == 0 and w3["stats"][2] > w["stats"][2]
    w4 = ref.network(a["coords"], a["box"], 3.5, COS30, min_bonds=4)
    assert w4["stats"][0] == w["stats"][0] and w4["stats"][1] == int((w["A"].sum(1) >= 4).sum())
    assert np.array_equal(w4["label"] >= 0, w["A"].sum(1) >= 4)


# ---- observables -------------------------------------------------------------------------------------
def stats_row(bonds, sizes, masks, flagged=False):
    if flagged:
        return [0] * 7 + [1]
    s = np.array(sizes)
    wrap = [x for x, mk in zip(sizes, masks) if mk]
    return [bonds, s.sum(), len(s), s.max(), (s * s).sum(), int(np.bitwise_or.reduce(masks)), max(wrap, default=0), 0]


def hand_made():
    """Three replicas, one criterion, N = 10: (6 wrapping xyz, 3, 1), (5 wrapping x, 5), flagged."""
    stats = np.array([[stats_row(9, [6, 3, 1], [7, 0, 0])], [stats_row(8, [5, 5], [1, 0])],
                      [stats_row(0, [], [], True)]], dtype=np.int64)
    hist = np.zeros((3, 1, 11), dtype=np.uint64)
    for s in (6, 3, 1):
        hist[0, 0, s] += 1
    hist[1, 0, 5] = 2
    return hist, stats


def test_observables_on_hand_made_histograms():
    hist, stats = hand_made()
    n_s, w_s = obs.cluster_size_distribution(hist.sum(0))
    assert n_s.shape == (1, 11) and n_s[0, 5] == 2 and n_s.sum() == 5
    assert np.allclose(w_s[0, [1, 3, 5, 6]], [0.05, 0.15, 0.5, 0.3]) and np.isclose(w_s.sum(), 1.0)
    p_any, p_all = obs.percolation_probability(stats)
    assert p_any.shape == (1,) and p_any[0] == 1.0 and p_all[0] == 0.5           # of the two unflagged
    g = obs.gel_fraction(stats)
    assert g.shape == (3, 1) and g[0, 0] == 0.6 and g[1, 0] == 0.5 and np.isnan(g[2, 0])
    # largest left out per replica: (3, 1) and one of the two fives
    want = (9 + 1 + 25) / (3 + 1 + 5)
    assert np.isclose(obs.mean_cluster_size(hist, stats)[0], want)
    assert np.isclose(obs.mean_cluster_size(hist.sum(0), stats)[0], want)
    one = np.array([[stats_row(0, [4], [0])]], dtype=np.int64)
    h1 = np.zeros((1, 5), dtype=np.uint64)
    h1[0, 4] = 1
    assert np.isnan(obs.mean_cluster_size(h1, one)[0])
    deg = np.zeros((2, 17), dtype=np.uint64)
    deg[0, [2, 3, 4]] = (1, 1, 2)
    f = obs.bond_fractions(deg)
    assert list(f[0, 2:5]) == [0.25, 0.25, 0.5] and np.all(np.isnan(f[1]))
    allflag = np.array([[stats_row(0, [], [], True)]], dtype=np.int64)
    assert np.isnan(obs.percolation_probability(allflag)[0][0])


def test_observables_refuse_wrong_shapes():
    hist, stats = hand_made()
    for bad in (np.zeros(()), np.zeros((3, 1))):
        with pytest.raises(ValueError):
            obs.cluster_size_distribution(bad)
    for fn in (obs.percolation_probability, obs.gel_fraction):
        for bad in (np.zeros((3, 7), dtype=np.int64), np.zeros(8, dtype=np.int64)):
            with pytest.raises(ValueError):
                fn(bad)
    for h, s in ((hist[:, 0], stats), (hist[:2], stats), (hist, stats[:, 0]), (np.zeros((2, 11)), stats)):
        with pytest.raises(ValueError):
            obs.mean_cluster_size(h, s)
    for bad in (np.zeros((2, 16)), np.zeros(())):
        with pytest.raises(ValueError):
            obs.bond_fractions(bad)
