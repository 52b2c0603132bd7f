"""Host side of the structure observables (observables.py: SLOT_PAIRS, fold_by_type,
normalize_rdf_pairs, dielectric_constant) and the numpy restatement of the six site-site rows the
GPU tests compare mmc_batch_rdf_sites with (tests/structure_ref.py)."""
import numpy as np
import pytest

import structure_ref as ref
from metropolismontecarlo_amd import observables as obs


def three_site_gas(n, side, seed):
    """n 'molecules' of three independent uniformly random sites: [3 n, 3], slot a at [a::3]."""
    return np.random.default_rng(seed).random((3 * n, 3)) * side


def test_slot_pairs_are_the_six_unordered_pairs_in_row_order():
    assert obs.SLOT_PAIRS == ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def test_restatement_of_the_six_rows():
    """Same-slot rows are numpy_check.make_rdf_hist of that slot; a cross row (a, b) counts every
    ordered molecule pair once: its total over an r_max that holds every image distance's bin is
    N (N - 1), and it equals the brute-force count of A[i] - B[j], i != j."""
    from oracle import numpy_check
    side, n, numbins = 9.0, 40, 17
    x = three_site_gas(n, side, 3)
    rows = ref.six_rows(x, side, numbins)
    for k, (a, b) in enumerate(obs.SLOT_PAIRS):
        if a == b:
            assert np.array_equal(rows[k], numpy_check.make_rdf_hist(x[a::3], side, numbins))
            continue
        A, B = x[a::3], x[b::3]
        d = A[:, None, :] - B[None, :, :]
        d = np.where(d < -side / 2, d + side, d)
        d = np.where(d > side / 2, d - side, d)
        rr = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        bins = np.ceil(rr / (side / 2 / numbins))[~np.eye(n, dtype=bool)]
        want = np.bincount(bins[bins <= numbins].astype(int), minlength=numbins + 1)
        assert np.array_equal(rows[k], want.astype(np.uint64))
    # a caller's r_max changes the bin width only
    r_max = 3.0
    rows2 = ref.six_rows(x, side, 10, r_max=r_max)
    d = x[0::3][:, None, :] - x[0::3][None, :, :]
    d -= side * np.round(d / side)
    rr = np.sqrt((d ** 2).sum(-1))[np.triu_indices(n, 1)]
    assert rows2[0].sum() == (rr <= r_max).sum()
    assert rows2[0][4] == ((rr > 3 * 0.3) & (rr <= 4 * 0.3)).sum()


def test_fold_by_type_for_spce_slots():
    h = np.arange(6 * 5, dtype=np.uint64).reshape(6, 5)
    rows, counts = obs.fold_by_type(h, ("O", "H", "H"))
    assert set(rows) == {("O", "O"), ("H", "O"), ("H", "H")}
    assert np.array_equal(rows[("O", "O")], h[0]) and counts[("O", "O")] == 1
    assert np.array_equal(rows[("H", "O")], h[1] + h[2]) and counts[("H", "O")] == 4
    assert np.array_equal(rows[("H", "H")], h[3] + h[4] + h[5]) and counts[("H", "H")] == 4
    # per-replica histograms fold along the last two axes; three distinct types keep six rows
    hr = np.stack([h, 2 * h])
    rows_r, _ = obs.fold_by_type(hr, ("O", "H", "H"))
    assert rows_r[("H", "H")].shape == (2, 5) and np.array_equal(rows_r[("H", "H")][1], 2 * rows[("H", "H")])
    rows3, counts3 = obs.fold_by_type(h, (1, 2, 3))
    assert len(rows3) == 6 and counts3[(1, 1)] == 1 and counts3[(1, 2)] == 2
    assert np.array_equal(rows3[(2, 3)], h[4])
    assert np.array_equal(h, np.arange(30, dtype=np.uint64).reshape(6, 5))    # the input is not modified


def test_normalize_rdf_pairs_on_an_ideal_gas_and_against_normalize_rdf():
    """The setup of test_host.test_rdf_restatement_and_normalisation_on_an_ideal_gas with three
    independent sites per point: every folded row gives g -> 1.

    Tolerance.  For independent uniform points the count of bin i is Poisson with mean
    mu_i = n_site_pairs 4 pi r_i^2 dr / V (the shell's share of the pairs).  The mean of g over bins
    i0..numbins is sum(c_i / mu_i) / m; with independent Poisson counts its variance is
    sum(1 / mu_i) / m^2 <= 1 / (m mu_min), mu_min the mean of the least-filled bin used (the
    innermost, i0).  Five such standard deviations are allowed: 5 / sqrt(m mu_min)."""
    side, n, numbins = 10.0, 1500, 25
    x = three_site_gas(n, side, 8)
    dr = side / 2 / numbins
    rows, counts = obs.fold_by_type(ref.six_rows(x, side, numbins), ("O", "H", "H"))
    i0 = 8
    m = numbins - i0
    for key, row in rows.items():
        n_pairs = counts[key] * n * (n - 1) / 2
        r_, g = obs.normalize_rdf_pairs(row, n_pairs, dr, 1.0 / side ** 3)
        assert np.allclose(r_[:2], [0.1, 0.3])
        mu_min = n_pairs * 4 * np.pi * r_[i0] ** 2 * dr / side ** 3
        tol = 5.0 / np.sqrt(m * mu_min)
        assert tol < 0.02, tol                      # (no weaker than the one-site test's 0.02)
        assert abs(g[i0:].mean() - 1.0) < tol, (key, g[i0:].mean(), tol)
    # a same-slot row: gr.jl divides by N^2 / 2 pairs where N (N - 1) / 2 are counted
    oo = rows[("O", "O")]
    _, g_old = obs.normalize_rdf(oo, n, side, 1)
    _, g_new = obs.normalize_rdf_pairs(oo, n * (n - 1) / 2, dr, 1.0 / side ** 3)
    assert np.allclose(g_new, g_old * n / (n - 1), rtol=1e-13, atol=0)
    # several frames at different volumes: sum of 1 / V
    _, g2 = obs.normalize_rdf_pairs(2 * oo.astype(float), n * (n - 1) / 2, dr, 2.0 / side ** 3)
    assert np.allclose(g2, g_new, rtol=1e-14)


def test_dielectric_constant_on_a_hand_made_series():
    # M alternates +-(1, 2, 2): <M> = 0, <M.M> = 9
    M = np.array([[1.0, 2.0, 2.0], [-1.0, -2.0, -2.0]] * 3)
    T, V, f = 300.0, 1000.0, 167101.0
    assert obs.dielectric_constant(M, T, V, f) == pytest.approx(1 + 4 * np.pi * f * 9 / (3 * V * T), rel=1e-14)
    # a constant offset does not fluctuate; volume per sample enters by its mean
    M2 = M + np.array([5.0, 0.0, -3.0])
    vols = np.array([900.0, 1100.0] * 3)
    assert obs.dielectric_constant(M2, T, vols, f) == pytest.approx(obs.dielectric_constant(M, T, V, f), rel=1e-12)
    assert obs.dielectric_constant(np.ones((4, 3)), T, V, f) == pytest.approx(1.0, abs=1e-12)


def test_restated_dipoles_do_not_see_broken_molecules():
    """vector1D of atom minus COM: an atom stored a box away from its COM gives the whole molecule's mu."""
    box = 12.0
    rng = np.random.default_rng(5)
    com = rng.random((6, 3)) * box
    off = (rng.random((6, 3, 3)) - 0.5) * 1.6
    coords = (com[:, None, :] + off).reshape(-1, 3)
    q = np.tile([-0.8476, 0.4238, 0.4238], 6)
    mu = ref.molecule_dipoles(com, coords, q, box)
    broken = coords.copy()
    broken[4] += [box, 0.0, -box]
    assert np.allclose(ref.molecule_dipoles(com, broken, q, box), mu, atol=1e-12)
    assert np.allclose(mu, np.einsum("ia,iad->id", q.reshape(6, 3), off), atol=1e-12)
