"""CPU tests around mmc_batch_deletion: the binning rule, the overlapping-distribution curves and
Bennett's acceptance ratio of observables.py, and -- on the oracle alone -- that the helper the GPU
tests compare against (deletion_ref.oracle_terms) agrees with the definition's other statement:
the deletion terms of molecule i in N are the insertion terms of i's coordinates into N without i."""
import math

import numpy as np
import pytest

import common
import deletion_ref as ref
from metropolismontecarlo_amd import observables as obs


# ---- energy_bins --------------------------------------------------------------------------------
def test_energy_bins_edges():
    n_bins, lo, hi = 4, 0.0, 2.0
    below_hi = np.nextafter(hi, -np.inf)
    du = np.array([lo, hi, below_hi, np.nan, np.nextafter(lo, -np.inf), -np.inf, np.inf, 1.0, -0.0, 1.999])
    h = obs.energy_bins(du, n_bins, lo, hi)
    assert h.dtype == np.uint64 and h.shape == (n_bins + 2,)
    assert h.sum() == du.size - 1                       # NaN is counted nowhere
    assert h[0] == 2                                    # just below u_lo, -inf
    assert h[1] == 2                                    # exactly u_lo and -0.0: the first bin
    assert h[n_bins + 1] == 2                           # exactly u_hi, +inf
    assert h[n_bins] == 2                               # the largest double below u_hi (k = 3.99.. -> 3), 1.999
    assert h[3] == 1                                    # 1.0: floor(1.0 * 2.0) = 2 -> slot 3
    assert np.array_equal(h, ref.energy_bins(du, n_bins, lo, hi))
    # a grid on which (below u_hi - u_lo) rounds to u_hi - u_lo: k = n_bins, the top slot by the rule
    n_bins, lo, hi = 10, -3.0, 2.0
    below_hi = np.nextafter(hi, -np.inf)
    assert below_hi < hi and (below_hi - lo) * (n_bins / (hi - lo)) == n_bins
    h = obs.energy_bins([below_hi, lo], n_bins, lo, hi)
    assert h[n_bins + 1] == 1 and h[1] == 1 and h.sum() == 2


def test_energy_bins_where_rounding_lifts_k_to_n_bins():
    """(dU - u_lo) * s can round up to n_bins for a dU below u_hi: the rule sends it to the top slot."""
    n_bins, lo, hi = 3, 0.0, 0.3
    s = np.float64(n_bins) / (np.float64(hi) - np.float64(lo))
    x = np.nextafter(hi, -np.inf)
    h = obs.energy_bins([x], n_bins, lo, hi)
    k = math.floor((x - lo) * s)
    assert h[n_bins + 1 if k >= n_bins else k + 1] == 1 and h.sum() == 1
    # ... on a seeded sweep of grids, against the scalar restatement
    rng = np.random.default_rng(5)
    for _ in range(200):
        n_bins = int(rng.integers(1, 4097))
        lo = float(rng.normal() * 1e4)
        hi = lo + float(rng.random() * 1e4 + 1e-3)
        edges = lo + (hi - lo) * rng.integers(0, n_bins + 1, size=20) / n_bins
        du = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf),
                             rng.uniform(lo - 10, hi + 10, size=40)])
        assert np.array_equal(obs.energy_bins(du, n_bins, lo, hi), ref.energy_bins(du, n_bins, lo, hi))


def test_energy_bins_refuses_a_bad_grid():
    for args in ((0, 0.0, 1.0), (5, 1.0, 1.0), (5, 2.0, 1.0), (5, float("nan"), 1.0), (5, 0.0, float("inf"))):
        with pytest.raises(ValueError):
            obs.energy_bins([0.5], *args)


# ---- overlap_curves -----------------------------------------------------------------------------
def test_overlap_curves_on_constructed_histograms():
    """f uniform on the grid, g = f exp(-(u - mu) / T) at the bin centres, both scaled to integers'
    worth of counts: the constant comes back as mu / T in every populated bin."""
    n_bins, lo, hi, T, mu = 8, -4.0, 4.0, 2.0, -1.25
    w = (hi - lo) / n_bins
    centres = lo + (np.arange(n_bins) + 0.5) * w
    f = np.full(n_bins, 1.0 / (hi - lo))
    g = f * np.exp(-(centres - mu) / T)
    n_ins, n_del = 4.0e6, 1.0e6
    h_ins = np.concatenate([[0.0], f * w * n_ins, [0.0]])
    # g has 0.97 of its mass on the grid: the rest sits in the top slot, and counts in the norm
    tail = n_del * (1.0 - (g * w).sum())
    assert tail > 0
    h_del = np.concatenate([[0.0], g * w * n_del, [tail]])
    c, ln_f, ln_g, const = obs.overlap_curves(h_ins, h_del, n_bins, lo, hi, T)
    assert np.allclose(c, centres, rtol=0, atol=1e-15)
    assert np.allclose(ln_f, np.log(f), rtol=0, atol=1e-12)
    assert np.allclose(const, mu / T, rtol=0, atol=1e-12)
    assert np.allclose(ln_g - ln_f + c / T, const, rtol=0, atol=1e-15)
    # empty bins: -inf in the curve, NaN in the constant, the rest unchanged
    h2 = h_ins.copy()
    h2[3] = 0.0
    _, ln_f2, _, const2 = obs.overlap_curves(h2, h_del, n_bins, lo, hi, T)
    assert ln_f2[2] == -np.inf and np.isnan(const2[2]) and np.isfinite(const2[[0, 1, 3, 4, 5, 6, 7]]).all()
    with pytest.raises(ValueError):
        obs.overlap_curves(h_ins[:-1], h_del, n_bins, lo, hi, T)


# ---- bennett_mu_ex ------------------------------------------------------------------------------
T_BAR, M_BAR, N_BAR = 300.0, -2000.0, 200000
S_BAR = 1.5 * T_BAR                                     # beta sigma = 1.5
MU_BAR = M_BAR - S_BAR * S_BAR / (2.0 * T_BAR)          # mu = m - beta sigma^2 / 2


def gaussian_pair(seed):
    """Insertion energies N(m, sigma^2) and their exact deletion partner N(m - beta sigma^2, sigma^2)."""
    rng = np.random.default_rng(seed)
    return (rng.normal(M_BAR, S_BAR, N_BAR), rng.normal(M_BAR - S_BAR * S_BAR / T_BAR, S_BAR, N_BAR))


def test_bennett_on_gaussian_energies():
    u_ins, u_del = gaussian_pair(1)
    mu, err = obs.bennett_mu_ex(u_ins, u_del, T_BAR)
    print("BAR", mu, "+-", err, "exact", MU_BAR)
    assert err > 0 and abs(mu - MU_BAR) <= 5 * err
    # the one-sided estimates of the same samples bracket nothing better
    widom = -T_BAR * math.log(np.exp(-u_ins / T_BAR).mean())
    inverse = T_BAR * math.log(np.exp(u_del / T_BAR).mean())
    assert abs(widom - MU_BAR) < 50 * err and abs(inverse - MU_BAR) < 50 * err
    # the returned error against the scatter over 20 seeds
    mus, errs = zip(*(obs.bennett_mu_ex(*gaussian_pair(100 + s), T_BAR) for s in range(20)))
    scatter = float(np.std(mus, ddof=1))
    print("scatter", scatter, "returned", float(np.mean(errs)))
    assert 0.5 * scatter <= err <= 2.0 * scatter
    assert abs(float(np.mean(mus)) - MU_BAR) <= 5 * scatter / math.sqrt(20)


def test_bennett_from_bin_centres_with_weights():
    u_ins, u_del = gaussian_pair(2)
    mu, err = obs.bennett_mu_ex(u_ins, u_del, T_BAR)
    n_bins, lo, hi = 4000, M_BAR - 12 * S_BAR, M_BAR + 12 * S_BAR
    h_ins, h_del = obs.energy_bins(u_ins, n_bins, lo, hi), obs.energy_bins(u_del, n_bins, lo, hi)
    assert h_ins[0] == h_ins[-1] == h_del[0] == h_del[-1] == 0
    centres = lo + (np.arange(n_bins) + 0.5) * (hi - lo) / n_bins
    mu_b, err_b = obs.bennett_mu_ex(centres, centres, T_BAR, w_ins=h_ins[1:-1], w_del=h_del[1:-1])
    assert abs(mu_b - mu) < 0.1 * err and abs(err_b - err) < 0.01 * err      # bins of 0.006 sigma
    # unequal sample sizes: M = ln(n_ins / n_del) enters
    mu_u, err_u = obs.bennett_mu_ex(u_ins, u_del[:N_BAR // 8], T_BAR)
    assert abs(mu_u - MU_BAR) <= 5 * err_u and err_u > err
    with pytest.raises(ValueError):
        obs.bennett_mu_ex(u_ins, [], T_BAR)
    with pytest.raises(ValueError):
        obs.bennett_mu_ex(u_ins, u_del, T_BAR, w_ins=np.ones(3))


# ---- the oracle-side identity -------------------------------------------------------------------
def test_sum_rules_on_the_oracle():
    """The relation the header states for esum: potential()'s lj and real count every pair once, the
    per-molecule terms count it from both sides."""
    from oracle import oracle
    from metropolismontecarlo_amd import structs
    a = common.nist_arrays(1, "unwrapped")
    s = common.oracle_system(a)
    L = a["box"]
    ew = oracle.Ewald(5.6 / L, 5, 27, L, factor=structs.factor)
    tot = oracle.potential_ewald(s, ew, 10.0, 10.0)
    lj = sum(oracle.lj_poly_du(i + 1, s, 10.0)[0] for i in range(s.n_mol))
    real = sum(oracle.ewald_short(i + 1, s, ew, 10.0)[0] for i in range(s.n_mol))
    assert common.rel(lj, 2 * tot["lj"]) < 1e-12 and common.rel(real, 2 * tot["real"]) < 1e-12


@pytest.mark.parametrize("variant", ["unwrapped", "reference"])
def test_deletion_terms_are_the_insertion_terms_into_the_rest(variant):
    from oracle import oracle
    a = common.nist_arrays(1, variant)
    L, rc = float(a["box"]), 10.0
    com, coords = np.asarray(a["com"]), np.asarray(a["coords"])
    for i in (0, 1, 37, 63, 64, 99):
        lj, real, recip, ov = ref.oracle_terms(oracle, a, com, coords, i, L, rc, rc)
        c0, x0 = ref.without(a, com, coords, i)
        assert c0.shape == (99, 3) and x0.shape == (297, 3)
        wlj, wreal, wrecip, wov, _ = common.widom_oracle_terms(oracle, a, c0, x0, ref.record(com, coords, i),
                                                               L, rc, rc)
        assert not ov and not wov
        # the same pairs in the same order (molecule i is skipped, or comes last): the pair terms
        # agree to the last bit or two; the reciprocal term is a difference of two sums of 1e3..1e4 K
        assert common.widom_close(lj, wlj) and common.widom_close(real, wreal), (i, lj, wlj, real, wreal)
        assert abs(recip - wrecip) <= 1e-9 + 1e-13 * abs(recip), (i, recip, wrecip)
        assert lj != 0.0 and real != 0.0 and recip < -1e4       # (the self term alone is -2.8e4 K)


def test_host_sums_follow_wave_sum_rows():
    """deletion_ref.wave_sum_rows: the scan inside rows of 16, then the rows in order."""
    v = np.arange(64, dtype=float) + 0.25
    assert ref.wave_sum_rows(v) == v.sum()                   # (exact in fp64 whatever the order)
    rng = np.random.default_rng(0)
    v = rng.normal(size=64) * 10.0 ** rng.integers(-8, 8, size=64)

    def row(x):                                              # lane 15 of a row after shifts 1, 2, 4, 8
        p = [x[k] + x[k - 1] for k in range(1, 16, 2)]       # pairs (1,0) (3,2) ..
        q = [p[k] + p[k - 1] for k in range(1, 8, 2)]
        r = [q[k] + q[k - 1] for k in range(1, 4, 2)]
        return r[1] + r[0]
    rows = [row(v[16 * k:16 * k + 16]) for k in range(4)]
    assert ref.wave_sum_rows(v) == ((rows[0] + rows[1]) + rows[2]) + rows[3]
    # flagged entries are skipped, lanes take entries l, l + 64, ...
    du = rng.normal(size=(1, 130, 3))
    ovl = np.zeros((1, 130), dtype=np.uint8)
    ovl[0, [5, 70]] = [1, 2]
    esum, boltz, nfl = ref.host_sums(du, ovl, 1.0, boltz0=[0.5], nflag0=[3])
    assert esum[0, 3] == 128 and nfl[0] == 5
    keep = ovl[0] == 0
    assert abs(esum[0, 0] - du[0, keep, 0].sum()) < 1e-12
    assert abs(boltz[0] - 0.5 - np.exp(du[0, keep].sum(1)).sum()) < 1e-10
