"""CPU tests of the spatial-distribution restatement (tests/sdf_ref.py) and of the host helpers
observables.sdf_density, sdf_unfold and sdf_cell_centres, on cases whose answer is known without a
computer: two molecules, one of them turned by a known rotation and the other placed at chosen
coordinates of its frame; and on the NIST fixtures."""
import numpy as np
import pytest

import common
import sdf_ref as sref
from metropolismontecarlo_amd import observables as obs

BOX = 32.0
N_HALF, CELL = 8, 0.5
# a water-like molecule in its own frame, every number dyadic: site 0 at the origin, sites 1 and 2 at
# (-+0.75, 0, 0.5), so that b = (0, 0, 1), h = (1.5, 0, 0) and the axes are the unit matrix, exactly
BODY = np.array([[0.0, 0.0, 0.0], [-0.75, 0.0, 0.5], [0.75, 0.0, 0.5]])
# proper rotations with entries 0 and +-1 (exact in fp64): rows are the images of x, y, z
ROTS = {
    "identity": np.eye(3),
    "x->y->z->x": np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]),
    "quarter turn about z": np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]),
    "half turn about x": np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]]),
}


def molecule(origin, rot):
    """BODY with its frame axes e_x, e_y, e_z = the rows of rot, site 0 at origin (wrapped into the box)."""
    return np.mod(np.asarray(origin, dtype=float) + BODY @ rot, BOX)


def cell_of(p, fold):
    """The grid index of frame coordinates p away from every edge, from the definition."""
    k = np.floor(np.asarray(p, dtype=float) / CELL).astype(int)
    ix = int(np.floor(abs(p[0]) / CELL)) if fold & 1 else k[0] + N_HALF
    iy = int(np.floor(abs(p[1]) / CELL)) if fold & 2 else k[1] + N_HALF
    return ix, iy, k[2] + N_HALF


def counts(coords, fold, site_mask=1, n_half=N_HALF, cell=CELL, box=BOX):
    flat = sref.sdf_counts(coords, box, n_half, cell, fold, site_mask)
    return flat[:-2].reshape(sref.grid_shape(n_half, fold)), int(flat[-2]), int(flat[-1])


def test_the_frame_of_a_turned_molecule_is_the_rotation():
    for name, rot in ROTS.items():
        s0, axes, off, ok = sref.frames(molecule((5.0, 6.0, 7.0), rot), BOX)
        assert ok.all() and np.array_equal(axes[0], rot), name
        assert np.array_equal(off[0], BODY @ rot), name
    # across a periodic face the molecule is whole
    s0, axes, off, ok = sref.frames(molecule((0.25, 31.875, 0.125), ROTS["x->y->z->x"]), BOX)
    assert ok.all() and np.array_equal(axes[0], ROTS["x->y->z->x"])


@pytest.mark.parametrize("name", sorted(ROTS))
@pytest.mark.parametrize("origin", [(5.0, 6.0, 7.0), (0.25, 31.5, 16.0)], ids=["inside", "across a face"])
def test_a_neighbour_lands_in_the_predicted_cell(name, origin):
    """Molecule 0 turned by a known rotation, the oxygen of molecule 1 at chosen coordinates p of
    0's frame (the second origin puts it across periodic faces).  +y and -y are told apart at fold 0:
    the handedness e_y = e_z x e_x.  Molecule 1 keeps the identity frame, so that molecule 0's oxygen
    sits at -(p.x e_x + p.y e_y + p.z e_z) of its frame: the deposit the other way."""
    rot = ROTS[name]
    for p in ((2.25, 0.75, 1.75), (2.25, -0.75, 1.75), (-1.25, 3.25, -2.75), (0.25, -0.25, 3.75)):
        p = np.array(p)
        other = np.asarray(origin) + p @ rot
        coords = np.concatenate([molecule(origin, rot), molecule(other, np.eye(3))])
        back = -(p @ rot)                                   # site 0 of molecule 0 in molecule 1's (identity) frame
        for fold in (0, 1, 2, 3):
            grid, outside, noframe = counts(coords, fold)
            want = np.zeros_like(grid)
            want[cell_of(p, fold)] += 1
            want[cell_of(back, fold)] += 1
            assert np.array_equal(grid, want) and outside == 0 and noframe == 0, (name, p, fold)
        assert cell_of(p, 0) != cell_of(p * (1, -1, 1), 0) and cell_of(p, 2) == cell_of(p * (1, -1, 1), 2)
    # the hydrogens of molecule 1 in molecule 0's frame, and beyond the cube
    p = np.array((2.25, 0.75, 1.75))
    coords = np.concatenate([molecule(origin, rot), molecule(np.asarray(origin) + p @ rot, rot)])
    grid, outside, noframe = counts(coords, 0, site_mask=6)
    want = np.zeros_like(grid)
    for a in (1, 2):
        want[cell_of(p + BODY[a], 0)] += 1
        want[cell_of(-p + BODY[a], 0)] += 1
    assert np.array_equal(grid, want) and outside == 0
    far = np.concatenate([molecule(origin, rot), molecule(np.asarray(origin) + np.array((4.25, 0.0, 0.0)) @ rot, rot)])
    grid, outside, noframe = counts(far, 3, site_mask=7)
    assert outside == 4 and grid.sum() == 2 and noframe == 0    # |x| = 4.25: only the site 0.75 nearer is in, each way


def test_degenerate_molecules_have_no_frame():
    good = molecule((5.0, 6.0, 7.0), np.eye(3))
    linear = np.array([[9.0, 6.0, 7.0], [9.75, 6.0, 7.0], [8.25, 6.0, 7.0]])       # o2 = -o1: b = 0
    collapsed = np.array([[5.0, 9.0, 7.0], [5.5, 9.0, 7.5], [5.5, 9.0, 7.5]])      # o1 = o2: h = 0
    for bad in (linear, collapsed):
        ok = sref.frames(np.concatenate([good, bad]), BOX)[3]
        assert ok.tolist() == [True, False]
    coords = np.concatenate([good, linear, collapsed])
    for mask, n_sel in ((1, 1), (6, 2), (7, 3)):
        grid, outside, noframe = counts(coords, 3, site_mask=mask)
        assert noframe == 2 * 2 * n_sel                       # each of the two sends its (N - 1) n_sel deposits there
        assert grid.sum() + outside == 2 * n_sel              # the good molecule sees both


def test_sum_rule_and_fixture_facts():
    for n_mol in (70, 100, 129, 200):
        # (as tests/test_gpu_sdf.py truncates them: configuration 1 holds 100 molecules, 2 holds 200)
        a = common.nist_arrays(1 if n_mol <= 100 else 2, "unwrapped")
        box = a["box"]
        assert box == 20.0
        coords = a["coords"][:3 * n_mol]
        assert sref.frames(coords, box)[3].all()              # every molecule has a frame
        assert not sref.on_an_edge(coords, box, N_HALF, CELL)
        for mask, n_sel in ((1, 1), (6, 2), (7, 3)):
            if n_mol > 100 and mask != 1:
                continue
            flat = sref.sdf_counts(coords, box, N_HALF, CELL, 3, mask)
            assert flat.sum() == n_mol * (n_mol - 1) * n_sel and flat[-1] == 0
        grid, outside, noframe = counts(coords, 3, box=box)
        top = np.unravel_index(np.argmax(grid), grid.shape)
        # the acceptor oxygen in front of a hydrogen: |x| in [2, 2.5), |y| < 0.5, z in [1.5, 2)
        assert top == (4, 0, 11), n_mol
        assert int(grid[top]) == {70: 19, 100: 28, 129: 48, 200: 85}[n_mol]
        if n_mol == 200:
            assert grid.sum() == 2612 and outside == 37188
            assert np.sort(grid.ravel())[-2] == 46


def test_folding_on_the_host_is_folding_in_the_pass():
    a = common.nist_arrays(2, "unwrapped")
    coords, box = a["coords"][:3 * 100], a["box"]
    assert not sref.on_an_edge(coords, box, N_HALF, CELL)     # the precondition: -e_k and e_k fold differently
    for mask in (1, 6):
        g0, out0, _ = counts(coords, 0, site_mask=mask, box=box)
        for fold in (1, 2, 3):
            g, out, _ = counts(coords, fold, site_mask=mask, box=box)
            assert np.array_equal(g, sref.fold_on_host(g0, fold)) and out == out0, (mask, fold)


def test_density_and_unfold():
    a = common.nist_arrays(1, "unwrapped")
    coords, box, n = a["coords"], a["box"], a["com"].shape[0]
    for fold in (0, 1, 2, 3):
        for mask, n_sel in ((1, 1), (7, 3)):
            grid, _, _ = counts(coords, fold, site_mask=mask, box=box)
            ideal = obs.sdf_ideal_count(n, 2, box ** 3, CELL, fold, mask)
            assert ideal == 2 * n * (n - 1) / box ** 3 * n_sel * CELL ** 3 * 2 ** bin(fold).count("1")
            g = obs.sdf_density(2 * grid, n, 2, box ** 3, CELL, fold, mask)
            assert g.shape == grid.shape and g.dtype == np.float64
            assert np.allclose(g * ideal, 2 * grid, rtol=1e-15, atol=0)
            full = obs.sdf_unfold(grid, fold)
            assert full.shape == (2 * N_HALF,) * 3 and full.sum() == grid.sum()
            if fold & 1:
                assert np.array_equal(full, full[::-1])
            if fold & 2:
                assert np.array_equal(full, full[:, ::-1])
            # the density of the unfolded grid at fold 0 is the density of the folded one, on both sides
            gu = obs.sdf_density(obs.sdf_unfold(grid, fold), n, 1, box ** 3, CELL, 0, mask)
            gf = obs.sdf_density(grid, n, 1, box ** 3, CELL, fold, mask)
            assert np.allclose(gu[N_HALF if fold & 1 else 0:, N_HALF if fold & 2 else 0:], gf, rtol=1e-15, atol=0)
            # a leading replica axis
            both = obs.sdf_unfold(np.stack([grid, 3 * grid]), fold)
            assert np.array_equal(both[0], full) and np.array_equal(both[1], 3 * full)
            x, y, z = obs.sdf_cell_centres(N_HALF, CELL, fold)
            assert (len(x), len(y), len(z)) == grid.shape
            assert z[0] == -3.75 and z[-1] == 3.75 and x[-1] == 3.75 and x[0] == (0.25 if fold & 1 else -3.75)
            assert y[0] == (0.25 if fold & 2 else -3.75)
    with pytest.raises(ValueError):
        obs.sdf_unfold(np.zeros((4, 4)), 3)
    with pytest.raises(ValueError):
        obs.sdf_density(np.zeros((4, 4, 4)), 10, 1, 1.0, 0.5, 4, 1)
    with pytest.raises(ValueError):
        obs.sdf_density(np.zeros((4, 4, 4)), 10, 1, 1.0, 0.5, 3, 0)
