"""The numpy restatement of mmc_batch_bond_order (tests/bond_order_ref.py) against an independent
form, and the frames the GPU tests use; no GPU.

The independent form has no spherical harmonics in it.  By the addition theorem
    q_l(i)^2 = sum over j, k in nb(i) of P_l(u_ij . u_ik) / n_i^2
    c_ij     = sum over k in nb(i), k' in nb(j) of P_l(u_ik . u_jk') / (n_i n_j)
               x (4 pi / (2 l + 1)) / (q_l(i) q_l(j))      [with q_l^2 = (4 pi / (2 l + 1)) Q the factor cancels]
with the Legendre polynomials from numpy.polynomial.  It is the authority for every known answer here;
the literature values quoted beside them are from memory.

What it gives (recorded from this test's own run, printed by it with -s):
    simple cubic   q4 = 0.763763, q6 = 0.353553     (literature 0.76376, 0.35355)
    fcc            q4 = 0.190941, q6 = 0.574524     (literature 0.19094, 0.57452)
    diamond        q3 = 0.745356, every c3 = -1
    wurtzite       the centre's eclipsed c3 = -0.111111 (literature about -0.11), its staggered c3 = -1"""
import numpy as np
import pytest

import bond_order_ref as ref
from metropolismontecarlo_amd import observables as obs
from shell_order_ref import random_frame

TOL = 1e-12


def check_against_legendre(a, p, some=None):
    out = ref.bond_order(a["coords"], a["box"], **p)
    n_mol = len(out["q"])
    for i in (range(n_mol) if some is None else some):
        if not out["defined"][i]:
            continue
        assert abs(out["q"][i] - ref.legendre_q(a["coords"], a["box"], out["nbr"], i, p["l"])) < TOL, i
        for k in range(out["n"][i]):
            j = out["nbr"][i, k]
            if np.isfinite(out["c"][i, k]):
                assert abs(out["c"][i, k] - ref.legendre_c(a["coords"], a["box"], out["nbr"], i, j, p["l"])) < TOL, (i, j)
    return out


@pytest.mark.parametrize("l", [3, 4, 6])
@pytest.mark.parametrize("n_mol,n_nb,r_nb", [(64, 4, 6.0), (129, 12, 8.0), (66, 16, 11.0)])
def test_restatement_equals_the_legendre_form_on_random_frames(l, n_mol, n_nb, r_nb):
    a = random_frame(n_mol)
    out = check_against_legendre(a, ref.params(l=l, n_nb=n_nb, r_nb=r_nb))
    assert out["defined"].sum() > n_mol // 2 and np.isfinite(out["c"]).sum() > n_mol
    assert np.nanmax(out["q"]) <= 1.0 + TOL and np.nanmax(np.abs(out["c"])) <= 1.0 + TOL


@pytest.mark.parametrize("l", [3, 4, 6])
def test_a_rigid_rotation_changes_nothing(l):
    """A non-periodic cluster (40 oxygens in the middle of a large box) turned about its centre."""
    rng = np.random.default_rng(12)
    O = 11.0 + (rng.random((40, 3)) - 0.5) * 7.0
    p = ref.params(l=l, n_nb=6, r_nb=4.0)
    x = ref.bond_order(ref.oxygen_frame(O, 22.0)["coords"], 22.0, **p)
    Orot = 11.0 + (O - 11.0) @ ref.rotation(5).T
    y = ref.bond_order(ref.oxygen_frame(Orot, 22.0)["coords"], 22.0, **p)
    assert np.array_equal(x["nbr"], y["nbr"]) and x["defined"].sum() > 30
    for k in ("q", "qbar", "c"):
        assert np.array_equal(np.isnan(x[k]), np.isnan(y[k])), k
        assert np.nanmax(np.abs(x[k] - y[k])) < TOL, k
    assert np.isfinite(x["qbar"]).sum() > 10 and np.isfinite(x["c"]).sum() > 60


def test_simple_cubic_and_fcc():
    a, r_nb = ref.sc_frame()
    q4 = check_against_legendre(a, ref.params(l=4, n_nb=6, r_nb=r_nb))["q"]
    q6 = check_against_legendre(a, ref.params(l=6, n_nb=6, r_nb=r_nb))["q"]
    print("simple cubic q4 %.6f q6 %.6f" % (q4[0], q6[0]))
    assert np.abs(q4 - 0.76376).max() < 1e-5 and np.abs(q6 - 0.35355).max() < 1e-5
    a, r_nb = ref.fcc_frame()
    out4 = check_against_legendre(a, ref.params(l=4, n_nb=12, r_nb=r_nb))
    out6 = check_against_legendre(a, ref.params(l=6, n_nb=12, r_nb=r_nb))
    print("fcc q4 %.6f q6 %.6f" % (out4["q"][0], out6["q"][0]))
    assert len(out6["q"]) == 32 and out6["stats"][3] == 0
    assert np.abs(out6["q"] - 0.57452).max() < 1e-5 and np.abs(out4["q"] - 0.19094).max() < 1e-5
    assert np.abs(out6["qbar"] - out6["q"]).max() < TOL         # every site has the same q_lm


def test_diamond_is_one_cluster_of_staggered_bonds():
    a, r_nb = ref.diamond_frame()
    out = check_against_legendre(a, ref.params(r_nb=r_nb))
    print("diamond q3 %.6f c3 %.6f .. %.6f" % (out["q"][0], np.nanmin(out["c"]), np.nanmax(out["c"])))
    c = out["c"][:, :4]
    assert len(out["q"]) == 64 and np.all(np.isfinite(c)) and np.all(c <= -0.8) and np.abs(c + 1.0).max() < TOL
    assert out["ab_hist"][4, 0] == 64 and out["ab_hist"].sum() == 64
    assert out["size_hist"][64] == 1 and out["size_hist"].sum() == 1 and np.all(out["label"] == 0)
    assert list(out["stats"]) == [64, 0, 0, 0, 64, 1, 64, 64 * 64]


def test_the_centre_of_a_wurtzite_fragment_is_hexagonal():
    a = ref.wurtzite_fragment()
    out = check_against_legendre(a, ref.params())
    assert len(out["q"]) == 17 and list(out["nbr"][0, :4]) == [1, 2, 3, 4]
    c = out["c"][0, :4]
    print("wurtzite centre c3", c)
    assert list(out["ab"][0]) == [3, 1]
    assert -0.35 <= c[0] <= 0.25 and abs(c[0] + 1.0 / 9.0) < 1e-9 and np.abs(c[1:] + 1.0).max() < 1e-9
    cls = obs.chill_plus_classes(dict(ab=out["ab"][None], nbr=out["nbr"][None]))
    assert cls.shape == (1, 6) and cls[0, 1] == 1 and cls.sum() == 17


def test_frames_of_the_gpu_tests_do_what_they_are_for():
    a = ref.line_frame()
    out = ref.bond_order(a["coords"], a["box"], **ref.params(n_nb=2, min_a=0, min_ab=0))
    assert out["size_hist"][128] == 1 and np.all(out["label"] == 0) and np.all(out["n"][1:-1] == 2)
    assert np.all(out["q"][1:-1] == 0.0) and np.all(np.isnan(out["c"][1:-1]))   # u and -u: odd l cancels exactly
    a = ref.bridging_frame()
    out = ref.bond_order(a["coords"], a["box"], **ref.params(n_nb=1, min_a=0, min_ab=0))
    nb = out["nbr"][:, 0]
    one_way = [(i, nb[i]) for i in range(12) if nb[nb[i]] != i]
    assert len(one_way) == 8 and list(out["label"]) == [0] * 6 + [6] * 6
    assert any(i < j for i, j in one_way) and any(i > j for i, j in one_way)      # pushed and pulled
    from shell_order_ref import coincident_frame
    a = coincident_frame()
    out = ref.bond_order(a["coords"], a["box"], **ref.params(r_nb=6.0))
    lonely = int(np.count_nonzero(out["n"] == 0))                  # a sparse frame: some have nobody inside r_nb
    assert not out["defined"][0] and not out["defined"][1] and out["n"][0] > 0 and out["stats"][1] == 2 + lonely
    assert np.isnan(out["q"][0]) and out["q_hist"][-1] == 2 + lonely and out["c_hist"][-1] >= out["n"][0] + out["n"][1]
    assert out["c_hist"][:-1].sum() > 0 and not np.any(np.isnan(out["q"][out["defined"]]))
    a = random_frame(129)
    out = ref.bond_order(a["coords"], a["box"], **ref.params(r_nb=11.0, n_nb=16, l=6))
    f = out["flagged"]
    assert 0 < f.sum() < 129 and np.any(out["used"] & f[np.maximum(out["nbr"], 0)] & ~f[:, None])  # a bond to a flagged one
    out = ref.bond_order(a["coords"], a["box"], **ref.params(r_nb=6.0))
    assert out["stats"][3] > 0


def test_observables_on_hand_made_results():
    h = np.zeros(5, np.uint64)
    h[[0, 3, 4]] = [1, 3, 4]
    q, p, und = obs.steinhardt_distribution(h)
    assert np.allclose(q, [0.125, 0.375, 0.625, 0.875]) and np.allclose(p, [1.0, 0, 0, 3.0]) and und == 0.5
    c, p, und = obs.bond_correlation_distribution(h)
    assert np.allclose(c, [-0.75, -0.25, 0.25, 0.75]) and np.allclose(p, [0.5, 0, 0, 1.5]) and und == 0.5
    stats = np.array([[6, 1, 1, 0, 4, 2, 3, 10], [8, 0, 0, 2, 0, 0, 0, 0]])
    assert np.allclose(obs.solid_fraction(stats), [0.5, 0.0]) and obs.solid_fraction(stats.sum(0)) == 0.25
    assert list(obs.largest_nucleus(stats)) == [3, 0]
    sh = np.array([0, 1, 0, 1], np.uint64)
    n_s, w_s = obs.nucleus_size_distribution(sh)
    assert np.allclose(n_s, [0, 1, 0, 1]) and np.allclose(w_s, [0, 0.25, 0, 0.75])
    with pytest.raises(ValueError):
        obs.solid_fraction(np.zeros((2, 7)))
    # one replica, eight molecules: S, E and the neighbours of each
    ab = np.array([[[4, 0], [3, 1], [0, 4], [1, 3], [2, 0], [2, 0], [3, 0], [1, 1]]], np.uint8)
    nbr = np.full((1, 8, 16), -1, np.int32)
    nbr[0, 4, :2] = [0, 7]      # S = 2 beside a cubic one: interfacial ice
    nbr[0, 5, :2] = [4, 7]      # S = 2, no neighbour above 2: liquid
    nbr[0, 6, :1] = [5]         # S = 3, E = 0 beside S = 2: interfacial ice
    cls = obs.chill_plus_classes(dict(ab=ab, nbr=nbr))
    assert cls.tolist() == [[1, 1, 2, 1, 1, 2]] and obs.CHILL_CLASSES[2] == "interfacial_ice"
