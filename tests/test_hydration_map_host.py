"""CPU tests of the hydration maps' restatement (tests/hydration_map_ref.py) against a plain double
loop over waters and sites, of its cell rule and roundings, and of the observables that turn
Batch.hydration_map's rows into densities, polarisations, energies and shell averages."""
import math

import numpy as np
import pytest

import hydration_map_ref as hm
import sdf_ref
import solute_ref as sr
from metropolismontecarlo_amd import observables

BOX = 20.0


def loop_image(x, box):
    if x > box / 2.0:
        return x - box
    if x < -box / 2.0:
        return x + box
    return x


def loop_cell(p, n_half, cell):
    """The cell of one coordinate by the header's words: k with e_k <= p < e_k+1, e_k = (double)k * cell,
    k = -n_half .. n_half - 1, stored at k + n_half; None in no cell."""
    for k in range(-n_half, n_half):
        if float(k) * cell <= p < float(k + 1) * cell:
            return k + n_half
    return None


def loop_v1d(c1, c2, box):
    d = c2 - c1
    if abs(d) < 0.5 * box:
        return d
    return d - math.copysign(1.0, d) * box


def loop_map(mol, coords, box, n_half, cell, u_lj, u_real, ov):
    """mmc_batch_hydration_map of one frame, a water and a site at a time in Python floats."""
    g, c = 2 * n_half, [float(v) for v in mol[-1]]
    cells = g ** 3
    out = [[0] * (cells + 2) for _ in range(8)]
    w = np.asarray(coords, dtype=float).reshape(-1, 3, 3)
    for j in range(w.shape[0]):
        where = []
        for a in range(3):
            idx = [loop_cell(loop_image(float(w[j, a, d]) - c[d], box), n_half, cell) for d in range(3)]
            where.append(cells if None in idx else (idx[0] * g + idx[1]) * g + idx[2])
            out[a][where[a]] += 1
        b = [loop_v1d(float(w[j, 0, d]), float(w[j, 1, d]), box) + loop_v1d(float(w[j, 0, d]), float(w[j, 2, d]), box)
             for d in range(3)]
        nb2 = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]
        if math.isfinite(nb2) and nb2 > 0.0:
            for d in range(3):
                out[3 + d][where[0]] += int(round(b[d] / math.sqrt(nb2) * 2.0 ** 30))     # (round(): ties to even)
        else:
            for d in range(3):
                out[3 + d][cells + 1] += 1
        us = (float(u_lj[j]), float(u_real[j]))
        if ov[j] or not all(math.isfinite(u) and abs(u) < 2.0 ** 20 for u in us):
            out[6][cells + 1] += 1
            out[7][cells + 1] += 1
        else:
            for k in range(2):
                out[6 + k][where[0]] += int(round(us[k] * 2.0 ** 20))
    return np.array(out, dtype=np.int64)


def random_frame(n, seed, box=BOX):
    """n waters of SPC/E-like geometry at random places and orientations, and energies to deposit."""
    rng = np.random.default_rng(seed)
    body = np.array([[0.0, 0.0, 0.0], [0.8165, 0.5774, 0.0], [-0.8165, 0.5774, 0.0]])
    coords = np.concatenate([rng.random(3) * box + body @ sr.rotation(rng).T for _ in range(n)])
    u_lj, u_real = rng.normal(size=n) * 300.0, rng.normal(size=n) * 2000.0
    return coords, u_lj, u_real, np.zeros(n, dtype=bool)


@pytest.mark.parametrize("n_half,cell", ((1, 0.5), (1, 10.0), (3, 1.7), (5, 0.7)))
def test_the_restatement_is_the_double_loop(n_half, cell):
    coords, u_lj, u_real, ov = random_frame(400, seed=n_half)
    u_lj[3], u_real[5], ov[7] = 2.0 ** 20, -np.inf, True                # three flagged waters
    u_lj[11] = np.nextafter(2.0 ** 20, 0.0)                             # ... and one just not
    o = np.rint(coords[3 * 20] * 64.0) / 64.0                           # a water whose O-H vectors cancel, exactly
    coords[3 * 20:3 * 20 + 3] = o, o + np.array([0.5, 0.25, 0.125]), o - np.array([0.5, 0.25, 0.125])
    mol = sr.placed(np.zeros((1, 3)), [BOX - 0.4, 0.3, BOX - 0.2])
    want = loop_map(mol, coords, BOX, n_half, cell, u_lj, u_real, ov)
    got = hm.hydration_map(mol, coords, BOX, n_half, cell, u_lj, u_real, ov)
    assert got.dtype == np.int64 and got.shape == (8, (2 * n_half) ** 3 + 2)
    assert (got == want).all()
    assert (got[:3].sum(1) == 400).all()                                # the tail-slot identity of the counts
    assert (got[6:, -1] == 3).all() and (got[:3, -1] == 0).all()
    assert (got[3:6, -1] == 1).all()                                    # the cancelling water
    if n_half > 1:                                                      # some inside, some outside
        assert got[0, :-2].sum() > 3 and got[0, -2] > 3
    assert (got[0, -2] == 0) == (cell == 10.0)                          # the cube that is the box holds every site


def test_the_cell_rule_on_edges_ends_and_nan():
    n_half, cell, c = 4, 0.5, np.array([19.5, 0.25, 19.75])
    mol = sr.placed(np.zeros((1, 3)), c)
    g = 2 * n_half
    body = np.array([[0.0, 0.0, 0.0], [0.25, 0.25, 0.0], [-0.25, 0.25, 0.0]])
    cases = {                                   # O's position relative to c -> its cell along x, None = outside
        (0.5, 0.25, 0.25): 5, (-2.0, 0.25, 0.25): 0, (2.0, 0.25, 0.25): None, (-0.0, 0.25, 0.25): 4,
        (float("nan"), 0.25, 0.25): None,
    }
    for off, ix in cases.items():
        coords = (c + np.array(off)) + body
        coords = coords - BOX * (coords[0] > BOX)       # the O in the box: the image brings it back, exactly
        sl = hm.slots(mol, coords, BOX, n_half, cell)
        want = g ** 3 if ix is None else (ix * g + 4) * g + 4
        assert sl[0, 0] == want, (off, sl)
        z = np.zeros(1)
        assert (hm.hydration_map(mol, coords, BOX, n_half, cell, z, z) == loop_map(mol, coords, BOX, n_half, cell, z, z, [False])).all()
        x = float(hm.image(coords[0, 0] - c[0], BOX))
        assert loop_cell(x, n_half, cell) == ix
    # the coordinates next to the cube's ends, and a cell that is no dyadic number
    for n_half, cell in ((4, 0.5), (7, 0.7), (12, 0.5)):
        e = np.arange(-n_half, n_half + 1).astype(float) * cell
        p = np.concatenate([e, np.nextafter(e, -100.0), np.nextafter(e, 100.0), [np.nan, np.inf, -np.inf]])
        k, inside = sdf_ref.cell_index(p, n_half, cell, False)
        assert [int(a) if b else None for a, b in zip(k, inside)] == [loop_cell(float(x), n_half, cell) for x in p]


def test_q30_and_q20_round_ties_to_even():
    for scale, f in ((2.0 ** 30, hm.VEC_SCALE), (2.0 ** 20, hm.E_SCALE)):
        assert f == scale
        v = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5000001, 0.49999999]) / scale
        assert hm.q_round(v, scale).tolist() == [0, 2, 2, 0, -2, -2, 4, 0]
    assert hm.q_round(1.0, 2.0 ** 30) == 2 ** 30 and hm.q_round(-(2.0 ** 20 - 2.0 ** -20), 2.0 ** 20) == -(2 ** 40 - 1)


def test_the_bisector_is_sdf_refs_e_z():
    coords = random_frame(300, seed=9)[0]
    ez, ok = hm.bisector(coords, BOX)
    _, axes, _, ok_sdf = sdf_ref.frames(coords, BOX)
    assert ok.all() and ok_sdf.all() and ez.tobytes() == axes[:, 2].tobytes()
    assert np.abs((ez * ez).sum(1) - 1.0).max() < 1e-15
    # a linear H-O..H has a bisector but no sdf frame; cancelling O-H vectors have neither
    lin = np.array([[1.0, 1.0, 1.0], [1.5, 1.0, 1.0], [2.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.5, 1.25, 1.0], [0.5, 0.75, 1.0]])
    ez, ok = hm.bisector(lin, BOX)
    assert ok.tolist() == [True, False] and sdf_ref.frames(lin, BOX)[3].tolist() == [False, False]
    assert ez[0].tolist() == [1.0, 0.0, 0.0]


def test_hydration_density_of_exact_ideal_gas_counts_is_one():
    n_half, cell, frames, n_mol, box = 6, 0.75, 64, 750, 28.2
    cells = (2 * n_half) ** 3
    row = np.zeros(cells + 2)
    row[:cells] = frames * n_mol / box ** 3 * cell ** 3
    g = observables.hydration_density(row, frames, n_mol, box ** 3, cell)
    assert g.shape == (12, 12, 12) and np.abs(g - 1.0).max() < 1e-12
    # a sampled gas through the restatement: every cell within 5 sigma of 1
    rng = np.random.default_rng(3)
    pts = rng.random((300000, 3)) * box
    mol = sr.placed(np.zeros((1, 3)), [1.0, box - 1.0, box / 2])
    m = hm.hydration_map(mol, np.repeat(pts, 3, axis=0), box, 2, 2.5)
    assert (m[0] == m[1]).all() and m[0].sum() == pts.shape[0]
    g = observables.hydration_density(m[0], 1, pts.shape[0], box ** 3, 2.5)
    expect = pts.shape[0] / box ** 3 * 2.5 ** 3
    assert np.abs(g - 1.0).max() < 5.0 / np.sqrt(expect)
    with pytest.raises(ValueError):
        observables.hydration_density(np.zeros(28), 1, 1, 1.0, 1.0)        # 26 cells are no cube


def test_hydration_polarisation_is_nan_exactly_on_empty_cells():
    rng = np.random.default_rng(4)
    n = rng.integers(0, 4, size=8 + 2)
    n[[1, 6]] = 0
    vec = np.zeros((3, 10), dtype=np.int64)
    vec[:, :8] = rng.integers(-2 ** 30, 2 ** 30, size=(3, 8)) * (n[:8] > 0)
    p = observables.hydration_polarisation(vec, n)
    assert p.shape == (2, 2, 2, 3)
    assert (np.isnan(p).all(-1).ravel() == (n[:8] == 0)).all() and (np.isnan(p).any(-1) == np.isnan(p).all(-1)).all()
    k = 3 if n[3] else 0
    assert np.allclose(p.reshape(8, 3)[k], vec[:, k] / 2.0 ** 30 / n[k], rtol=1e-15)
    # a cell whose two waters both point along +z
    vec[:, 0], n[0] = (0, 0, 2 * 2 ** 30), 2
    assert observables.hydration_polarisation(vec, n)[0, 0, 0].tolist() == [0.0, 0.0, 1.0]


def test_hydration_energy_per_water_and_per_volume():
    n = np.array([2, 0, 1, 4, 0, 0, 3, 1, 5, 0])
    u = np.zeros((2, 10), dtype=np.int64)
    u[0, :8] = np.array([-300, 0, 50, 80, 0, 0, -9, 1]) * 2 ** 20
    u[1, :8] = np.array([-700, 0, -50, 20, 0, 0, 9, 1]) * 2 ** 20
    per_water, per_vol = observables.hydration_energy(u, n, 0.5, frames=4)
    assert per_water.shape == per_vol.shape == (2, 2, 2)
    assert per_water.ravel()[[0, 2, 3, 6, 7]].tolist() == [-500.0, 0.0, 25.0, 0.0, 2.0]
    assert np.isnan(per_water.ravel()[[1, 4, 5]]).all()
    assert per_vol.sum() * 0.5 ** 3 == (u[:, :8].sum() / 2 ** 20) / 4          # the cube's share of <u_sw> per frame
    one, _ = observables.hydration_energy(u[0], n, 0.5, frames=4)
    assert one.ravel()[0] == -150.0


def test_hydration_radial_average_of_a_uniform_map_is_uniform():
    n_half, cell, dr = 8, 0.5, 0.4
    cells = (2 * n_half) ** 3
    row = np.full(cells + 2, 7, dtype=np.int64)
    r, mean, cnt = observables.hydration_radial_average(row, n_half, cell, dr)
    assert r.shape == mean.shape == cnt.shape == (10,) and np.allclose(r, (np.arange(10) + 0.5) * dr)
    assert cnt[0] == 0 and np.isnan(mean[0])                   # no centre within 0.4 of the origin (the nearest: 0.43)
    assert (mean[cnt > 0] == 7.0).all() and cnt[1] == 8 and cnt.sum() <= cells
    # shells of cell centres: a map that is its own radius averages to the shell's mean radius
    c = observables.hydration_map_centres(n_half, cell)
    assert c.shape == (16, 16, 16, 3) and c[0, 0, 0].tolist() == [-3.75] * 3 and c[8, 7, 15].tolist() == [0.25, -0.25, 3.75]
    rr = np.sqrt((c * c).sum(-1))
    _, mean, cnt = observables.hydration_radial_average(rr, n_half, cell, dr)
    k = np.arange(10)
    assert ((mean >= k * dr) & (mean < (k + 1) * dr))[cnt > 0].all()
    # NaN cells (an empty cell of a polarisation, say) are skipped
    rr[8, 8, 8] = np.nan
    assert observables.hydration_radial_average(rr, n_half, cell, dr)[2][1] == 7
