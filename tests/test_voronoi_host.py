"""CPU tests that pin tests/voronoi_ref.py, the numpy restatement of mmc_batch_voronoi that the GPU
tests compare with bit for bit: against scipy's Voronoi cells of 27 periodic images, on the four
lattices with known cells, and on the invariants of a tessellation.  The flag counts of the NIST
fixtures are asserted as conditions of the GPU tests that use them, not as measurements."""
import numpy as np
import pytest

import voronoi_ref as ref


nist_cells, lattice_cells = ref.nist_cells, ref.lattice_cells


def same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def scipy_cells(coords, box):
    """(V, S, faces) [N] of the periodic Voronoi cells from scipy on 27 images."""
    spatial = pytest.importorskip("scipy.spatial")
    O = np.asarray(coords)[0::3]
    n = len(O)
    shifts = [(0, 0, 0)] + [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)]
    pts = np.concatenate([O + box * np.array(s, float) for s in shifts])
    vor = spatial.Voronoi(pts)
    V, S = np.empty(n), np.empty(n)
    for i in range(n):
        region = vor.regions[vor.point_region[i]]
        assert -1 not in region and len(region) >= 4
        hull = spatial.ConvexHull(vor.vertices[region])
        V[i], S[i] = hull.volume, hull.area
    faces = np.bincount(vor.ridge_points[(vor.ridge_points < n)], minlength=n)[:n]
    return V, S, faces


@pytest.mark.parametrize("k,r_list", [(3, 6.0), (4, 7.5)])
def test_against_scipy_on_27_images(k, r_list):
    """V, S and the face counts of every cell the restatement certifies, within 1e-10 relative (its
    own worst was 2.1e-14 when it was prototyped: the margin is for the hull's arithmetic)."""
    pytest.importorskip("scipy")
    a, out, _ = nist_cells(k, "unwrapped", r_list)
    V, S, faces = scipy_cells(a["coords"], a["box"])
    ok = out["faces"] >= 0
    assert ok.sum() >= 0.95 * len(ok)
    assert np.abs(out["vol"][ok] / V[ok] - 1.0).max() < 1e-10
    assert np.abs(out["area"][ok] / S[ok] - 1.0).max() < 1e-10
    assert np.array_equal(out["faces"][ok], faces[ok])


def test_fixture_conditions():
    """Configuration 3 at 6.0 A: nothing flagged, in both COM variants.  Configuration 4 at 7.5 A: no
    CAP, no POLY, OPEN for at most 5 % (the largest cells of a box at 0.83 g/cm^3)."""
    for variant in ("unwrapped", "reference"):
        _, out, _ = nist_cells(3, variant, 6.0)
        assert not out["flagged"].any() and out["sums"][0] == 300, variant
    _, out, stats = nist_cells(4, "unwrapped", 7.5)
    cap, opened, poly = (int(v) for v in out["flagged"])
    assert cap == 0 and poly == 0 and 0 < opened <= 0.05 * 750
    assert np.all(out["faces"][out["faces"] < 0] == -ref.F_OPEN)
    assert stats["max_vertices"] <= 13                       # far from MAXV on water


@pytest.mark.parametrize("name", list(ref.LATTICES))
def test_lattices(name):
    n, a, basis, r_list, eta, faces, per_cell = ref.LATTICES[name]
    arr, out = lattice_cells(name, 1e-6)
    assert not out["flagged"].any()
    assert np.abs(out["vol"] / (a ** 3 / per_cell) - 1.0).max() < 1e-12
    assert np.abs(out["eta"] - eta).max() < 1e-7            # the table's digits
    assert np.abs(out["eta"] / out["eta"][0] - 1.0).max() < 1e-12
    # a cube; a truncated octahedron of edge 1 (S = 6 + 12 sqrt 3, V = 8 sqrt 2); a rhombic
    # dodecahedron of edge 1 (S = 8 sqrt 2, V = 16 sqrt 3 / 9); diamond's triakis truncated tetrahedron
    # at a = 1: four hexagons of 3 sqrt 3 / 16 towards the nearest neighbours and twelve triangles of
    # sqrt 2 / 64 towards the second ones, V = 1 / 8
    exact = {"sc": 6.0 / np.pi, "bcc": (6.0 + 12.0 * 3.0 ** 0.5) ** 3 / (36.0 * np.pi * 128.0),
             "fcc": (8.0 * 2.0 ** 0.5) ** 3 / (36.0 * np.pi * (16.0 * 3.0 ** 0.5 / 9.0) ** 2),
             "diamond": ((12.0 * 3.0 ** 0.5 + 3.0 * 2.0 ** 0.5) / 16.0) ** 3 / (36.0 * np.pi / 64.0)}[name]
    assert np.abs(out["eta"] - exact).max() < 1e-12
    assert np.all(out["faces"] == faces)
    assert out["face_hist"][faces] == len(out["vol"]) and out["face_hist"].sum() == len(out["vol"])
    assert abs(out["vol"].sum() / arr["box"] ** 3 - 1.0) < 1e-12
    _, raw = lattice_cells(name, 0.0)
    assert same_bits(raw["vol"], out["vol"]) and same_bits(raw["area"], out["area"])   # every face enters V and S
    if name in ("sc", "diamond"):
        assert raw["faces"].max() > faces                    # degenerate faces: what area_min is for
    else:
        assert np.all(raw["faces"] >= faces)


def test_total_volume_is_the_box_when_nothing_is_flagged():
    for variant in ("unwrapped", "reference"):
        a, out, _ = nist_cells(3, variant, 6.0)
        assert abs(out["vol"].sum() / a["box"] ** 3 - 1.0) < 1e-12
        assert abs(out["sums"][1] / a["box"] ** 3 - 1.0) < 1e-12
    a, out = lattice_cells("diamond", 1e-6, 0.3)
    assert not out["flagged"].any() and abs(out["vol"].sum() / a["box"] ** 3 - 1.0) < 1e-12


def test_geometric_neighbours_are_mutual_on_a_jittered_lattice():
    _, out = lattice_cells("diamond", 1e-6, 0.3)
    nbr = [set(int(j) for j in row if j >= 0) for row in out["nbr"]]
    assert all(len(s) == f for s, f in zip(nbr, out["faces"]))
    for i, s in enumerate(nbr):
        for j in s:
            assert i in nbr[j], (i, j)
    # ... and a shared face has one area, to rounding
    for i, s in enumerate(nbr):
        for j in s:
            ai = out["face_area"][i][list(out["nbr"][i]).index(j)]
            aj = out["face_area"][j][list(out["nbr"][j]).index(i)]
            assert abs(ai - aj) <= 1e-10 * max(ai, 1.0), (i, j)


def test_sums_follow_the_per_molecule_values():
    a, out, _ = nist_cells(4, "unwrapped", 7.5)
    ok = out["faces"] >= 0
    s = out["sums"]
    assert s[0] == ok.sum() and s[5] == out["faces"][ok].sum() and s[7] == 0.0
    assert abs(s[1] - out["vol"][ok].sum()) < 1e-9 and abs(s[2] - (out["vol"][ok] ** 2).sum()) < 1e-7
    assert abs(s[3] - out["area"][ok].sum()) < 1e-9 and abs(s[4] - out["eta"][ok].sum()) < 1e-10
    assert abs(s[6] - out["face_area"][ok].sum()) < 1e-9
    assert out["side_hist"].sum() == s[5] == out["nbr_hist"].sum()
    assert out["vol_hist"].sum() == out["eta_hist"].sum() == out["face_hist"].sum() == s[0]
    assert 3.0 * out["side_hist"][3] + sum(k * int(out["side_hist"][k]) for k in range(4, 17)) == pytest.approx(
        (6.0 - 12.0 / (s[5] / s[0])) * s[5], rel=1e-12)        # Euler, three faces at every vertex


FRAMES = [("nist", 3, "unwrapped", 6.0), ("nist", 3, "reference", 6.0), ("nist", 4, "unwrapped", 7.5),
          ("lattice", "sc", 0.0), ("lattice", "bcc", 0.0), ("lattice", "fcc", 0.0), ("lattice", "diamond", 0.0),
          ("lattice", "diamond", 0.3)]


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "-".join(str(x) for x in f))
def test_the_pruning_rule_changes_no_bit(frame):
    if frame[0] == "nist":
        with_rule, without = nist_cells(*frame[1:])[1], nist_cells(*frame[1:], prune=False)[1]
    else:
        with_rule, without = lattice_cells(frame[1], 1e-6, frame[2])[1], lattice_cells(frame[1], 1e-6, frame[2], prune=False)[1]
    for k in with_rule:
        assert same_bits(with_rule[k], without[k]), k


def test_small_frames_and_a_coincident_pair():
    """The frames of the GPU tests' flag paths: two and three molecules are OPEN, 66 in a ball are
    CAP, both molecules of a coincident pair are OPEN."""
    for n_mol in (2, 3):
        a = ref.random_frame(n_mol)
        out = ref.voronoi(a["coords"], a["box"], r_list=0.5 * ref.BOX)
        assert out["flagged"][1] == n_mol and np.all(out["faces"] == -ref.F_OPEN) and not out["sums"].any()
    a = ref.ball_frame(66)
    out = ref.voronoi(a["coords"], a["box"])
    assert out["flagged"][0] == 66 and np.all(out["faces"] == -ref.F_CAP) and np.all(np.isnan(out["vol"]))
    a = ref.ball_frame(65)
    out = ref.voronoi(a["coords"], a["box"])
    # the list filled exactly: the inner cells of the cluster are closed, those at its surface open
    assert out["flagged"][0] == 0 and 0 < out["flagged"][1] < 65 and out["sums"][0] == 65 - out["flagged"][1]
    a = ref.coincident_frame()
    out = ref.voronoi(a["coords"], a["box"], r_list=0.5 * ref.BOX)
    assert out["faces"][0] == -ref.F_OPEN and out["faces"][1] == -ref.F_OPEN


def test_a_ring_of_tangent_planes_reaches_maxv_and_passes_it():
    """The synthetic polygon of the POLY path: 16 tangent planes leave the two faces towards the
    close pair with MAXV = 16 sides and the cell whole; 17 flag it POLY (and only that: its other
    faces still close it)."""
    a = ref.ring_frame(16)
    stats = {}
    out = ref.voronoi(a["coords"], a["box"], r_list=ref.RING_R_LIST, mols=[0], stats=stats)
    assert out["faces"][0] == 18 and out["side_hist"][16] == 2 and out["side_hist"][4] == 16 and stats["max_vertices"] == 16
    assert abs(out["vol"][0] - 2.0 * 16 * 2.5 ** 2 * np.tan(np.pi / 16)) < 1e-12       # the prism
    a = ref.ring_frame(17)
    out = ref.voronoi(a["coords"], a["box"], r_list=ref.RING_R_LIST, mols=[0])
    assert out["faces"][0] == -ref.F_POLY and out["flagged"][2] == 1 and np.isnan(out["vol"][0])
