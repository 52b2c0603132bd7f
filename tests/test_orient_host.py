"""CPU tests of the orientation restatement (tests/orient_ref.py) and of the host helpers
observables.kirkwood_gk and orient_projections, on cases whose answer is known without a computer:
lattices of parallel and alternating molecules, one pair along and across its axes."""
import numpy as np

import common
import orient_ref as oref
import structure_ref as sref
from metropolismontecarlo_amd import observables as obs

UNIT = 2 ** 30
Q = (-1.0, 0.5, 0.5)
# a neutral three-site molecule whose dipole is exactly (1, 0, 0) e A: every number is dyadic, so all
# of mu, n^2 and u are exact
OFF = np.array([[0.0, 0.0, 0.0], [1.0, 0.75, 0.0], [1.0, -0.75, 0.0]])
BOX = 32.0


def molecules(site0, signs):
    """Molecules with site 0 at `site0` [N, 3] and axis sign (+-1) x: (com, coords, charge)."""
    site0, signs = np.asarray(site0, dtype=float), np.asarray(signs, dtype=float)
    coords = (site0[:, None, :] + signs[:, None, None] * OFF[None]).reshape(-1, 3)
    com = coords.reshape(-1, 3, 3).mean(1)        # (any reference point does for a neutral molecule)
    return com, coords, np.tile(Q, site0.shape[0])


def lattice(n_side, spacing=4.0):
    g = np.arange(n_side) * spacing + 1.0
    return np.array([(x, y, z) for x in g for y in g for z in g])


def test_row_0_is_the_site_0_histogram_of_the_structure_restatement():
    a = common.nist_arrays(1, "unwrapped")
    box = a["box"]
    n = a["com"].shape[0]
    for numbins, r_max in ((50, 0.0), (1, 0.0), (37, 7.5)):
        rows = oref.orient_rows(a["com"], a["coords"], a["charge"], box, numbins, r_max)
        want = sref.six_rows(a["coords"], box, numbins, r_max)[0]
        assert rows.dtype == np.int64 and rows.shape == (4, numbins + 2)
        assert np.array_equal(rows[0, :-1], want.astype(np.int64))
        assert rows[0, -1] == n * (n - 1) // 2 - int(want.sum())
        assert rows[2, -1] == 0 and rows[3, -1] == 0
        assert np.array_equal(rows, oref.orient_rows(a["com"], a["coords"], a["charge"], box, numbins, r_max,
                                                     reverse=True))
    u = oref.axes(a["com"], a["coords"], a["charge"], box)
    assert np.all(np.abs(oref.dot3(u, u) - 1.0) < 1e-15)


def test_parallel_lattice():
    s0 = lattice(3)
    com, coords, q = molecules(s0, np.ones(27))
    assert np.array_equal(oref.axes(com, coords, q, BOX), np.tile([1.0, 0.0, 0.0], (27, 1)))
    rows = oref.orient_rows(com, coords, q, BOX, 20, 10.0)
    assert rows[0].sum() == 27 * 26 // 2 and rows[0, -1] > 0 and rows[0, :-1].sum() > 0
    assert np.array_equal(rows[1], UNIT * rows[0])                # c = 1 for every pair
    assert np.array_equal(rows[3, :-1], UNIT * rows[0, :-1])      # p2 = 1
    assert rows[3, -1] == 0 and rows[2, -1] == 0
    gk = obs.kirkwood_gk(rows, 27)
    assert gk.shape == (22,) and gk[-1] == 27.0                   # |sum u|^2 / N = N
    assert np.all(np.diff(gk) >= 0)


def test_antiparallel_lattice():
    s0 = lattice(3)
    signs = np.array([1.0 if (i + j + k) % 2 == 0 else -1.0 for i in range(3) for j in range(3) for k in range(3)])
    com, coords, q = molecules(s0, signs)
    u = oref.axes(com, coords, q, BOX)
    assert np.array_equal(u[:, 0], signs)
    numbins = 12
    rows = oref.orient_rows(com, coords, q, BOX, numbins, 4.5)   # dr = 0.375: nearest neighbours (4.0) in bin 11
    nn = rows[0, 11]
    assert nn == 54 and rows[1, 11] == -UNIT * nn                 # unlike pairs only: c = -1
    assert np.array_equal(rows[3, :-1], UNIT * rows[0, :-1])      # p2 = 1 either way
    # 14 up, 13 down: |sum u|^2 / N = 1 / 27
    tot = u.sum(0)
    gk = obs.kirkwood_gk(rows, 27)
    assert abs(gk[-1] - float(tot @ tot) / 27) < 1e-12 and abs(gk[-1] - 1.0 / 27) < 1e-12
    assert gk[11] == 1.0 - 2.0 * 54 / 27
    # a leading replica axis, and two frames
    both = np.stack([rows, rows])
    assert np.array_equal(obs.kirkwood_gk(both, 27), np.stack([gk, gk]))
    assert np.allclose(obs.kirkwood_gk(both.sum(0), 27, n_frames=2), gk, rtol=0, atol=1e-15)


def test_one_pair_along_and_across_its_axes():
    for sep, hd in (((3.0, 0.0, 0.0), 2), ((0.0, 3.0, 0.0), -1), ((0.0, 0.0, -3.0), -1)):
        s0 = np.array([[5.0, 5.0, 5.0], np.add((5.0, 5.0, 5.0), sep)])
        rows = oref.orient_rows(*molecules(s0, [1.0, 1.0]), BOX, 8, 4.0)       # dr = 0.5: r = 3 is bin 6
        want = np.zeros((4, 10), dtype=np.int64)
        want[:, 6] = (1, UNIT, hd * UNIT, UNIT)
        assert np.array_equal(rows, want), sep
        # antiparallel axes: c = -1, hd = -3 + 1 along, +1 across
        rows = oref.orient_rows(*molecules(s0, [1.0, -1.0]), BOX, 8, 4.0)
        want[:, 6] = (1, -UNIT, -hd * UNIT, UNIT)
        assert np.array_equal(rows, want), sep
    # the same pair through the periodic boundary, and beyond r_max: rows 0 and 1 only
    s0 = np.array([[1.0, 5.0, 5.0], [30.0, 5.0, 5.0]])
    rows = oref.orient_rows(*molecules(s0, [1.0, 1.0]), BOX, 8, 4.0)
    assert rows[:, 6].tolist() == [1, UNIT, 2 * UNIT, UNIT]
    rows = oref.orient_rows(*molecules(s0, [1.0, 1.0]), BOX, 8, 2.0)
    assert rows[:, 9].tolist() == [1, UNIT, 0, 0] and rows[:, :9].sum() == 0
    # coincident sites: hd = 0; a molecule without a dipole: u = 0
    s0 = np.array([[5.0, 5.0, 5.0], [5.0, 5.0, 5.0]])
    rows = oref.orient_rows(*molecules(s0, [1.0, 1.0]), BOX, 8, 4.0)
    assert rows[:, 0].tolist() == [1, UNIT, 0, UNIT]
    com, coords, q = molecules(np.array([[5.0, 5.0, 5.0], [8.0, 5.0, 5.0]]), [1.0, 1.0])
    q[3:] = 0.0
    assert np.array_equal(oref.axes(com, coords, q, BOX)[1], np.zeros(3))
    rows = oref.orient_rows(com, coords, q, BOX, 8, 4.0)
    assert rows[:, 6].tolist() == [1, 0, 0, -UNIT // 2]


def test_orient_projections():
    a = common.nist_arrays(2, "unwrapped")
    box, n, numbins = a["box"], a["com"].shape[0], 40
    rows = oref.orient_rows(a["com"], a["coords"], a["charge"], box, numbins)
    dr = (box / 2) / numbins
    r, g, h110, h112, p2 = obs.orient_projections(rows, n, dr, 1.0 / box ** 3)
    six = sref.six_rows(a["coords"], box, numbins)
    r_oo, g_oo = obs.normalize_rdf_pairs(six[0], n * (n - 1) / 2, dr, 1.0 / box ** 3)
    assert np.array_equal(r, r_oo) and np.array_equal(g, g_oo)
    assert all(x.shape == (numbins,) for x in (r, g, h110, h112, p2))
    empty = rows[0, 1:-1] == 0
    assert empty.any() and not empty.all()
    assert np.array_equal(np.isnan(p2), empty)
    assert np.all(np.abs(h110) <= g + 1e-15) and np.all(np.abs(h112) <= 2 * g + 1e-15)
    assert np.all((p2[~empty] >= -0.5) & (p2[~empty] <= 1.0))
    full = ~empty
    assert np.allclose(h110[full] / g[full], rows[1, 1:-1][full] / (UNIT * rows[0, 1:-1][full]), rtol=1e-14)
    # a leading replica axis
    r2, g2, h2, k2, p22 = obs.orient_projections(np.stack([rows, 2 * rows]), n, dr, 1.0 / box ** 3)
    assert g2.shape == (2, numbins) and np.array_equal(g2[0], g) and np.array_equal(g2[1], 2 * g)
    assert np.array_equal(h2[0], h110) and np.array_equal(k2[0], h112)
    assert np.array_equal(np.isnan(p22[1]), empty) and np.allclose(p22[1][full], p2[full], rtol=1e-15)
