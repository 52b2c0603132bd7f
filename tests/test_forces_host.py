"""CPU tests around mmc_batch_forces: the numpy restatement the GPU tests compare against
(forces_ref.molecule) is pinned on the oracle by central differences of the reference's own energy,
the virial by equality, the header's sum rule on the oracle's totals, and the host observables on
hand-made sums.

The differenced energy is what the definition names (include/mmc_hip.h): with the stored COM array
frozen, U_i = orc.lj_poly_du(i) + orc.ewald_short(i) + factor orc.recip_long(all atoms) -- every term
of potential(..., "ewald") that depends on an atom of molecule i, each pair once.

Finite-difference tolerance (not fixed in advance): every difference is taken at h and at h / 2;
their disagreement plus eps |U_i| / h (rounding of the energies, |U_i| the sum of the three terms'
magnitudes, eps = 2^-52) is the finite difference's own error, and the test allows 10 times that.
Record of one run (h = 1e-4 A, theta = 1e-4 rad; both NIST configurations, molecules 0, 63, 64 and
N - 1): the worst |fd - ref| / allowed was 0.14 for the atom forces and 0.10 for the torques; the
allowed error itself was 2e-6 .. 3e-3 K/A.  No molecule needed the skip rule."""
import numpy as np
import pytest

import common
import forces_ref as ref
from metropolismontecarlo_amd import observables as obs
from metropolismontecarlo_amd import structs

RCUT = 10.0
H = 1.0e-4          # A, and rad for the rotations
EPS = 2.0 ** -52
MASS = (15.9994, 1.00794, 1.00794)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


class Energy:
    """U_i of one molecule of one configuration on the oracle, the stored COM frozen."""

    def __init__(self, orc, a):
        self.orc, self.a = orc, a
        self.L = float(a["box"])
        self.n = np.asarray(a["com"]).shape[0]
        self.ew = orc.Ewald(5.6 / self.L, 5, 27, self.L, factor=structs.factor)
        self.q = np.asarray(a["charge"], dtype=float)

    def system(self, coords):
        a = self.a
        return self.orc.System(a["com"], a["first_atom"], a["last_atom"], coords, a["atype"], a["charge"],
                               a["eps"], a["sig"], self.L)

    def terms(self, coords, i):
        s = self.system(coords)
        lj, _ = self.orc.lj_poly_du(i + 1, s, RCUT)
        real, _, ov = self.orc.ewald_short(i + 1, s, self.ew, RCUT)
        assert not ov
        rec = self.ew.factor * self.orc.recip_long(self.ew, coords, self.q, self.L)
        return lj, real, rec

    def __call__(self, coords, i):
        lj, real, rec = self.terms(coords, i)
        return (lj + real) + rec

    def S(self, coords):
        self.orc.recip_long(self.ew, coords, self.q, self.L)
        return self.ew.sumQExpOld.copy()


def central(u, x0, move, i, h):
    """(derivative, its own error): central differences of u along `move` at h and h / 2."""
    def diff(s):
        return (u(move(x0, +s), i) - u(move(x0, -s), i)) / (2 * s)
    d1, d2 = diff(h), diff(0.5 * h)
    return d2, abs(d1 - d2)


def rotation(axis, theta):
    n = np.zeros(3)
    n[axis] = 1.0
    K = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    return np.eye(3) + np.sin(theta) * K + (1 - np.cos(theta)) * (K @ K)


@pytest.mark.parametrize("cfg", [1, 4])
def test_forces_and_torques_against_central_differences_of_the_oracle(orc, cfg):
    a = common.nist_arrays(cfg, "unwrapped")
    en = Energy(orc, a)
    com, x0 = np.asarray(a["com"], dtype=float), np.asarray(a["coords"], dtype=float).reshape(-1, 3)
    su = ref.setup(a, orc, en.L, RCUT, RCUT)
    S = en.S(x0)
    listed = [0, 63, 64, en.n - 1]
    skipped, worst_f, worst_t, allowed_seen = 0, 0.0, 0.0, []
    for i in listed:
        r = ref.molecule(su, com, x0, S, i, MASS)
        assert not r["overlap"]
        if not ref.fd_safe(r, 2 * H):
            skipped += 1
            continue
        mag = sum(abs(t) for t in en.terms(x0, i))
        noise = EPS * mag / (0.5 * H)
        for at in range(3):
            for d in range(3):
                def move(x, s, at=at, d=d):
                    y = x.copy()
                    y[3 * i + at, d] += s
                    return y
                du, err = central(en, x0, move, i, H)
                allowed = 10 * (err + noise)
                allowed_seen.append(allowed)
                ratio = abs(-du - r["atom"][at, d]) / allowed
                worst_f = max(worst_f, ratio)
                assert ratio <= 1.0, (cfg, i, at, d, -du, r["atom"][at, d], allowed)
        for axis in range(3):
            def turn(x, s, axis=axis):
                y = x.copy()
                dd = ref.vector1D(com[i][None, :], x[3 * i:3 * i + 3], en.L)
                y[3 * i:3 * i + 3] = x[3 * i:3 * i + 3] + (dd @ rotation(axis, s).T - dd)
                return y
            du, err = central(en, x0, turn, i, H)
            allowed = 10 * (err + noise)
            ratio = abs(-du - r["torque"][axis]) / allowed
            worst_t = max(worst_t, ratio)
            assert ratio <= 1.0, (cfg, i, axis, -du, r["torque"][axis], allowed)
        # F and tau are the restated combinations of the per-atom forces
        assert np.allclose(r["force"], r["atom"].sum(0), rtol=0, atol=1e-12 * r["A_force"].max())
        assert np.allclose(r["torque"], np.cross(r["d"], r["atom"]).sum(0), rtol=0, atol=1e-12 * r["A_torque"].max())
        # the virial is the reference's own number
        _, vir = orc.lj_poly_du(i + 1, en.system(x0), RCUT)
        assert common.rel(r["vir"][0], vir) < 1e-12, (i, r["vir"][0], vir)
        assert r["vir"][2] > 0 and np.isfinite(r["vir"][1])
    print(f"config {cfg}: h = {H}, worst ratio forces {worst_f:.3g} torques {worst_t:.3g}, "
          f"allowed {min(allowed_seen):.3g} .. {max(allowed_seen):.3g}, skipped {skipped}")
    assert 10 * skipped <= len(listed)


def test_virial_sum_rule_on_the_oracle(orc):
    """The factor the header states: potential()'s virial halves the sum over molecules of
    LJ_poly_dU's vir (energy.jl:978-980) and carries a third of every Coulomb term besides."""
    a = common.nist_arrays(1, "unwrapped")
    s = common.oracle_system(a)
    L = float(a["box"])
    ew = orc.Ewald(5.6 / L, 5, 27, L, factor=structs.factor)
    tot = orc.potential_ewald(s, ew, RCUT, RCUT)
    w = sum(orc.lj_poly_du(i + 1, s, RCUT)[1] for i in range(s.n_mol))
    assert common.rel(w, 2 * (tot["virial"] - tot["coulomb"] / 3.0)) < 1e-12
    # ... and the restatement's w_lj sums to the same, its forces to zero
    su = ref.setup(a, orc, L, RCUT, RCUT)
    com, x0 = np.asarray(a["com"], dtype=float), np.asarray(a["coords"], dtype=float).reshape(-1, 3)
    orc.recip_long(ew, x0, np.asarray(a["charge"], dtype=float), L)
    S = ew.sumQExpOld.copy()
    rows = [ref.molecule(su, com, x0, S, i) for i in range(s.n_mol)]
    assert common.rel(sum(r["vir"][0] for r in rows), w) < 1e-12
    F, A = sum(r["force"] for r in rows), sum(r["A_force"] for r in rows)
    assert np.all(np.abs(F) <= 1e-12 * A), (F, A)
    assert all(r["vir"][2] == 0.0 for r in rows)            # no mass: t = 0


def test_a_linear_arrangement_has_a_singular_inertia_tensor(orc):
    a = common.nist_arrays(1, "unwrapped")
    L = float(a["box"])
    su = ref.setup(a, orc, L, RCUT, RCUT)
    com, x = np.asarray(a["com"], dtype=float).copy(), np.asarray(a["coords"], dtype=float).reshape(-1, 3).copy()
    x[0:3] = com[0] + np.array([[0.0, 0, 0], [0.5, 0, 0], [-0.5, 0, 0]])
    with np.errstate(all="ignore"):
        r = ref.molecule(su, com, x, np.zeros(337, dtype=complex), 0, MASS)
    assert not np.isfinite(r["vir"][2])


def test_host_sums_order():
    rng = np.random.default_rng(2)
    F, T, W = rng.normal(size=(2, 130, 3)), rng.normal(size=(2, 130, 3)), rng.normal(size=(2, 130, 3))
    ovl = np.zeros((2, 130), dtype=np.uint8)
    ovl[1, [5, 70]] = [1, 2]
    F[1, [5, 70]] = T[1, [5, 70]] = W[1, [5, 70]] = 0.0
    fsum, nfl = ref.host_sums(F, T, W, ovl, nflag0=[3, 4])
    assert fsum[0, 0] == 130 and fsum[1, 0] == 128 and list(nfl) == [3, 6]
    assert abs(fsum[0, 1] - (F[0] ** 2).sum()) < 1e-11 and abs(fsum[0, 2] - (T[0] ** 2).sum()) < 1e-11
    assert np.allclose(fsum[1, 4:7], F[1].sum(0), atol=1e-12) and abs(fsum[1, 3] - W[1, :, 2].sum()) < 1e-12
    assert abs(fsum[1, 7] - W[1, :, 0].sum()) < 1e-12 and abs(fsum[1, 8] - W[1, :, 1].sum()) < 1e-12
    # lane 0 of a replica adds entries 0, 64, 128 in that order
    assert fsum[0, 4] == ref.wave_sum_rows([(F[0, l, 0] + F[0, l + 64, 0]) + (F[0, l + 128, 0] if l < 2 else 0.0)
                                            for l in range(64)])


# ---- observables --------------------------------------------------------------------------------
def test_mean_square_force_on_hand_made_sums():
    fsum = np.array([[4.0, 40.0, 8.0, 2.0, 0, 0, 0, 0, 0], [2.0, 10.0, 6.0, 3.0, 0, 0, 0, 0, 0]])
    r = obs.mean_square_force(fsum)
    assert np.array_equal(r["f2"], [10.0, 5.0]) and np.array_equal(r["tau2"], [2.0, 3.0])
    assert np.array_equal(r["t"], [0.5, 1.5])
    assert r["f2_pooled"] == 50.0 / 6.0 and r["tau2_pooled"] == 14.0 / 6.0 and r["t_pooled"] == 5.0 / 6.0
    se = np.std([10.0, 5.0], ddof=1) / np.sqrt(2)
    assert abs(r["f2_err"] - se) < 1e-15
    one = obs.mean_square_force(fsum[:1])
    assert one["f2_pooled"] == 10.0 and np.isnan(one["f2_err"])
    with pytest.raises(ValueError):
        obs.mean_square_force(np.zeros((2, 8)))
    empty = obs.mean_square_force(np.zeros((1, 9)))
    assert np.isnan(empty["f2"][0])


def test_quantum_correction_constant_and_formula():
    # hbar^2 / (k_B amu A^2) in K: CODATA 2018 exact hbar and k_B, amu = 1.66053906660e-27 kg
    hbar, kb, amu = 1.054571817e-34, 1.380649e-23, 1.66053906660e-27
    c = hbar * hbar / (kb * amu * 1e-20)
    assert abs(obs.HBAR2_OVER_KB_AMU_A2 - c) <= 1e-12 * c and abs(c - 48.5087) < 1e-3
    fsum = np.array([[5.0, 5.0 * 3.0e6, 0.0, 5.0 * 2.0e5, 0, 0, 0, 0, 0]])
    T, mass = 300.0, (16.0, 1.0, 1.0)
    r = obs.quantum_correction(fsum, T, mass)
    want = c / (24.0 * T * T) * (3.0e6 / 18.0 + 2.0e5)
    assert abs(r["dA"] - want) <= 1e-14 * want and abs(r["per_replica"][0] - want) <= 1e-14 * want
    assert abs(r["translational"] - c / (24 * T * T) * 3.0e6 / 18.0) <= 1e-14 * want
    with pytest.raises(ValueError):
        obs.quantum_correction(fsum, 0.0, mass)
    with pytest.raises(ValueError):
        obs.quantum_correction(fsum, T, (16.0, 0.0, 1.0))
