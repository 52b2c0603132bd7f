"""CPU tests of the shell-order restatement (tests/shell_order_ref.py) on frames with closed-form
answers, of the normalisations in observables.py, and of what the inputs of the GPU tests
(tests/test_gpu_shell_order.py) cover -- asserted here, on the restatement alone."""
import numpy as np
import pytest

import shell_order_ref as ref
from metropolismontecarlo_amd import observables as obs


@pytest.mark.parametrize("n,a", [(4, 5.5), (5, 4.5)])
def test_simple_cubic_lattice_in_closed_form(n, a):
    fr = ref.lattice_frame(n, a)
    p = ref.lattice_params(a)
    o = ref.shell_order(fr["coords"], fr["box"], **p)
    N = n ** 3
    assert o["flagged"] == 0 and np.all(o["count"] == 18)          # 6 at a, 12 at a sqrt(2)
    assert np.all(o["n_lsi"] == 6) and np.all(o["m_ang"] == 6) and np.all(o["ties"])
    # five gaps of exactly zero and one of a (sqrt(2) - 1): mean = g / 6, I = (5 mean^2 + (g - mean)^2) / 6
    g = a * (np.sqrt(2.0) - 1.0)
    assert np.allclose(o["lsi"], 5.0 * g * g / 36.0, rtol=1e-13, atol=0.0)
    assert len(set(o["lsi"].view(np.uint64))) == 1                 # the spacings are exact: so is every r^2
    # 15 pairs: 12 at cos 0, 3 at cos -1
    nb = p["ang_bins"]
    assert o["ang_hist"][nb // 2] == 12 * N and o["ang_hist"][0] == 3 * N and o["ang_hist"].sum() == 15 * N
    # ranks 1..6 in one bin, 7 and 8 in another
    kb = int(np.floor(a * (p["r_bins"] / p["r_list"])))
    assert np.all(o["rank_hist"][:6, kb] == N) and np.all(o["rank_hist"][6:, kb] == 0)
    assert np.all(o["rank_hist"].sum(1) == N)
    # ties resolved by j: the six at r^2 = a a exactly, in rising index
    _, r2 = ref.oo_vectors(fr["coords"], fr["box"])
    for i in range(N):
        assert list(o["nbr"][i, :6]) == sorted(np.flatnonzero(r2[i] == a * a)), i
        assert list(o["nbr"][i, 6:]) == sorted(np.flatnonzero(r2[i] == 2 * a * a))[:10], i


def test_pentamer_has_four_bonds_and_a_known_zeta():
    fr = ref.pentamer_frame()
    o = ref.shell_order(fr["coords"], fr["box"])
    assert o["count"][0] == 5 and o["n_bonded"][0] == 4
    assert list(o["nbr"][0, :6]) == [1, 2, 3, 4, 5, -1]
    assert abs(o["zeta"][0] - (ref.PENTAMER_FAR - ref.PENTAMER_R)) < 1e-12
    assert o["n_bonded"][5] == 0 and np.isnan(o["zeta"][5])         # nobody bonds to the sixth
    # the centre's angles: six tetrahedral ones (cos = -1/3) and those to the sixth molecule
    o = ref.shell_order(fr["coords"], fr["box"], r_ang=3.0, ang_bins=3)
    assert o["m_ang"][0] == 4 and o["ang_hist"][1] >= 6


def test_lsi_by_hand():
    rho = np.array([2.7, 2.8, 3.0, 3.4, 4.1])
    d = np.diff(rho)
    assert ref.lsi_of(rho, 4) == pytest.approx(np.mean((d - d.mean()) ** 2), rel=1e-13)
    assert ref.lsi_of(rho, 1) == 0.0


def test_bins_clamp():
    assert ref.clamp_bin(-0.5, 9) == 0 and ref.clamp_bin(9.99, 9) == 9 and ref.clamp_bin(np.inf, 9) == 9
    assert ref.clamp_bin(3.999, 9) == 3 and ref.clamp_bin(-np.inf, 9) == 0
    assert list(ref.lsi_bin([0.0, 0.39, 0.4, 7.0, np.nan], 4, 0.4)) == [0, 3, 3, 3, 4]
    assert list(ref.zeta_bin([-9.0, -1.5, 0.49, 0.5, 2.5, np.nan], 4, -1.5, 2.5)) == [0, 0, 1, 2, 3, 4]


# ---- observables --------------------------------------------------------------------------------------
def test_distance_lsi_and_zeta_densities_integrate_to_one():
    rng = np.random.default_rng(0)
    h = rng.integers(1, 50, size=(3, 8, 31)).astype(np.uint64)
    r, p, beyond = obs.neighbour_distance_distributions(h, 6.0)
    assert r.shape == (30,) and p.shape == (3, 8, 30) and beyond.shape == (3, 8)
    assert np.allclose(r[[0, -1]], [0.1, 5.9]) and np.allclose(p.sum(-1) * 0.2, 1.0)
    assert np.allclose(beyond, h[..., 30] / h.sum(-1))
    x, p, und = obs.lsi_distribution(h[0, 0], 0.3)
    assert np.allclose(x[[0, -1]], [0.005, 0.295]) and np.isclose(p.sum() * 0.01, 1.0) and np.isclose(und, h[0, 0, 30] / h[0, 0].sum())
    x, p, und = obs.zeta_distribution(h[1], -1.0, 2.0)
    assert np.allclose(x[[0, -1]], [-0.95, 1.95]) and np.allclose(p.sum(-1) * 0.1, 1.0) and und.shape == (8,)
    # one value in one bin: the density is 1 / width there
    one = np.zeros(11, np.uint64)
    one[3] = 5
    x, p, und = obs.zeta_distribution(one, 0.0, 5.0)
    assert p[3] == 2.0 and p.sum() == 2.0 and und == 0.0
    with pytest.raises(ValueError):
        obs.neighbour_distance_distributions(np.zeros(5), 6.0)


def test_angle_distribution_carries_the_jacobian():
    nb = 180
    iso = np.full(nb + 1, 1000, np.uint64)                          # uniform in cos(theta): isotropic
    iso[nb] = 17                                                     # the non-finite slot is left out
    theta, p, mc = obs.ooo_angle_distribution(iso)
    edges = np.degrees(np.arccos(np.linspace(-1.0, 1.0, nb + 1)))[::-1]
    assert np.all(np.diff(theta) > 0) and np.allclose(theta, 0.5 * (edges[:-1] + edges[1:]))
    assert np.isclose((p * np.diff(edges)).sum(), 1.0) and abs(mc) < 1e-12
    mid = slice(10, nb - 10)                                         # P(theta) = sin(theta) / 2 per radian
    assert np.allclose(p[mid], 0.5 * np.sin(np.radians(theta[mid])) * np.pi / 180.0, rtol=2e-3)
    # all angles tetrahedral
    h = np.zeros((2, nb + 1), np.uint64)
    h[:, int(np.floor((-1.0 / 3.0 + 1.0) * nb / 2.0))] = 9
    theta, p, mc = obs.ooo_angle_distribution(h)
    k = int(np.argmax(p[0]))
    assert abs(theta[k] - 109.47) < 0.6 and np.allclose(mc, -1.0 / 3.0, atol=1.0 / nb) and p.shape == (2, nb)


def test_means_from_the_sums():
    s = np.array([[1.0, 4.0, -3.0, 6.0], [0.0, 0.0, 2.0, 1.0]])
    assert np.allclose(obs.lsi_mean(s), [0.25, np.nan], equal_nan=True)
    assert np.allclose(obs.zeta_mean(s), [-0.5, 2.0])
    assert obs.lsi_mean(s.sum(0)) == 0.25
    with pytest.raises(ValueError):
        obs.zeta_mean(np.zeros((3, 2)))


# ---- what the GPU tests' inputs cover -------------------------------------------------------------------
def case(n_mol, name, r=0):
    a = ref.random_frame(n_mol)
    return ref.shell_order(ref.replica_frame(a, r)[1], a["box"], **ref.CASES[name])


def test_gpu_inputs_cover_the_cap():
    full, over = ref.ball_frame(65), ref.ball_frame(66)
    o = ref.shell_order(full["coords"], ref.BOX)
    assert o["flagged"] == 0 and np.all(o["count"] == 64)           # exactly full, every molecule
    o = ref.shell_order(over["coords"], ref.BOX)
    assert o["flagged"] == 66 and np.all(o["count"] == -1) and o["rank_hist"].sum() == 0
    for r in range(3):                                               # some flagged, some not; a list of exactly 64
        o = case(129, "L/2", r)
        assert 0 < o["flagged"] < 129, r
    o = case(129, "L/2")
    assert o["count"].max() == 64
    # a list that crosses 64 in the second pass of the lanes, and one that does so only with j = 128
    _, r2 = ref.oo_vectors(ref.random_frame(129)["coords"], ref.BOX)
    near = r2 < (0.5 * ref.BOX) ** 2
    np.fill_diagonal(near, False)
    upto128 = near[:, :128].sum(1)
    assert np.any((near[:, :64].sum(1) <= 64) & (upto128 > 64))
    assert np.any((upto128 == 64) & near[:, 128])
    for n_mol in (2, 3, 64, 65, 66):
        assert case(n_mol, "L/2")["flagged"] == 0


def test_gpu_inputs_cover_undefined_lsi_and_zeta_both_ways():
    o = case(129, "3.7")
    ok = o["count"] >= 0
    assert np.any(o["n_lsi"] == 0) and np.any((o["n_lsi"] > 0) & np.isnan(o["lsi"]) & ok)   # none inside; n + 1 missing
    assert np.any(np.isfinite(o["lsi"]))
    assert np.any(o["n_bonded"] == 0)                                                       # no bond
    assert np.any((o["n_bonded"] > 0) & (o["n_bonded"] == o["count"]))                      # nobody else listed
    assert np.any(np.isfinite(o["zeta"]))
    o = case(129, "7")
    assert np.all(np.isfinite(o["lsi"])) and np.isfinite(o["zeta"]).sum() > 100
    assert o["zeta_hist"][0] > 0 and o["zeta_hist"][6] > 0 and o["lsi_hist"][6] > 0         # the clamps at both ends
    assert o["rank_hist"][15].sum() == 129 and 0 < o["rank_hist"][15, 7] < 129              # some without a 16th


def test_gpu_inputs_cover_ties_and_a_coincident_oxygen():
    for n_mol in ref.SIZES:
        for name in ref.CASES:
            assert not case(n_mol, name)["ties"].any()              # the random frames have none: the lattice has
    fr = ref.coincident_frame()
    o = ref.shell_order(fr["coords"], fr["box"], r_list=7.0, r_ang=7.0)
    assert o["nbr"][0, 0] == 1 and o["nbr"][1, 0] == 0 and o["ang_hist"][-1] > 0
    assert o["ties"].any()                                          # molecules 0 and 1 are equally far from a third
