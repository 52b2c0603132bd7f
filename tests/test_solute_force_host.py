"""CPU tests around mmc_batch_solute_forces: the numpy restatement the GPU tests compare against
(solute_force_ref.replica) is pinned on the oracle by central differences of the reference's own energy,
and the host observables on hand-made numbers.

The differenced energy is what the definition names (include/mmc_hip.h): with the stored reference point c
and all COMs frozen, U = orc.lj_poly_du(N + 1) + orc.ewald_short(N + 1) + factor orc.recip_long(all N + 1
molecules) + orc.ewald_self(the solute's charges) -- every term of potential(..., "ewald") of the N + 1
system that depends on the solute, each pair once.  Site forces: every site component moved by +-h;
torque: the sites rotated about c; phi: q_a shifted by +-delta; field: the q_a-derivative of the site
force (exact: the force is linear in q_a), for every site of the solutes with at most five sites and for
every uncharged site.

Finite-difference tolerance (test_forces_host.py's rule, not fixed in advance): every difference is taken
at h and at h / 2; their disagreement plus eps |U| / h (rounding of the energies, |U| the sum of the four
terms' magnitudes, eps = 2^-52) is the finite difference's own error, and the test allows 10 times that.
Record of one run (h = 1e-4 A, theta = 1e-4 rad, delta = 1e-3 e; 65 waters of NIST configuration 1, all
fourteen placements): the worst |fd - ref| / allowed was 0.18 for the site forces, 0.27 for the torques,
0.080 for phi and 0.13 for the fields; the allowed error itself was 4e-7 .. 1.4e-2 K/A, and 2.4e-6 ..
5.7e-2 K/(e A) for the fields, which difference two finite differences.  No placement needed the skip rule."""
import numpy as np
import pytest

import common
import solute_force_ref as ref
import solute_ref as sr
from metropolismontecarlo_amd import observables as obs
from metropolismontecarlo_amd import structs

H = 1.0e-4          # A, and rad for the rotations
DQ = 1.0e-3         # e
DQ_FIELD = 0.25     # e: the two charges between which the site force is differenced for the field
EPS = 2.0 ** -52
N_WATER = 65


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def water():
    return sr.first_molecules(common.nist_arrays(1, "unwrapped"), N_WATER)


class Energy:
    """U of one placement on the oracle; the waters, c and every COM frozen."""

    def __init__(self, orc, a, sol, lj_rcut, qq_rcut):
        self.orc, self.sol = orc, sol
        self.so = sr.SoluteOracle(orc, a, sol, lj_rcut, qq_rcut)
        self.L = float(a["box"])
        self.com = np.asarray(a["com"], dtype=float)
        self.x = np.asarray(a["coords"], dtype=float).reshape(-1, 3)
        self.n, self.S = self.com.shape[0], sol.n_sites
        self.q_w = np.asarray(a["charge"][:3 * self.n], dtype=float)
        self.ew = orc.Ewald(5.6 / self.L, 5, 27, self.L, factor=structs.factor)

    def terms(self, mol, q):
        n, S, so = self.n, self.S, self.so
        first = np.concatenate([3 * np.arange(n, dtype=np.int64) + 1, [3 * n + 1]])
        last = np.concatenate([3 * np.arange(n, dtype=np.int64) + 3, [3 * n + S]])
        atype = np.concatenate([np.tile([1, 2, 3], n), 4 + np.arange(S)]).astype(np.int64)
        q1 = np.concatenate([self.q_w, q])
        s = self.orc.System(np.vstack([self.com, mol[S]]), first, last, np.vstack([self.x, mol[:S]]), atype, q1,
                            so.eps, so.sig, self.L)
        lj, _ = self.orc.lj_poly_du(n + 1, s, so.lj_rcut)
        real, _, ov = self.orc.ewald_short(n + 1, s, self.ew, so.qq_rcut)
        assert not ov
        rec = self.ew.factor * self.orc.recip_long(self.ew, s.coords, q1, self.L)
        return lj, real, rec, self.orc.ewald_self(self.ew, q)

    def __call__(self, mol, q):
        lj, real, rec, slf = self.terms(mol, q)
        return ((lj + real) + rec) + slf

    def S_k(self, mol, q):
        self.terms(mol, q)
        return self.ew.sumQExpOld.copy()


def central(u, h):
    """(derivative, its own error) of u(s) at 0: central differences at h and h / 2."""
    d1, d2 = (u(h) - u(-h)) / (2 * h), (u(0.5 * h) - u(-0.5 * h)) / h
    return d2, abs(d1 - d2)


def rotation(axis, theta):
    n = np.zeros(3)
    n[axis] = 1.0
    K = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    return np.eye(3) + np.sin(theta) * K + (1 - np.cos(theta)) * (K @ K)


def placement(a, sol, seed, corner=False, clear=2.3):
    """The solute rotated at random, its reference point drawn in the box (or within 0.3 A of the corner
    at the origin) until no site is closer than `clear` to a water atom."""
    rng = np.random.default_rng(seed)
    L, x = float(a["box"]), np.asarray(a["coords"], dtype=float).reshape(-1, 3)
    for _ in range(20000):
        c = (rng.random(3) - 0.5) * 0.6 % L if corner else rng.random(3) * L
        mol = sr.placed(sol.offsets, c, sr.rotation(rng))
        d = mol[:-1, None, :] - x[None, :, :]
        d -= L * np.rint(d / L)
        if (d * d).sum(2).min() > clear * clear:
            return mol
    raise AssertionError("no placement found")


def solutes(a):
    return {"cation": sr.cation(a), "dipole": sr.dipole(a), "methane": sr.methane(a), "synthetic5": sr.synthetic(a, 5, 3),
            "synthetic16": sr.synthetic(a, 16, 7), "mea": sr.mea()}


CASES = [(name, cut, seed, False) for name in ("cation", "dipole", "methane", "synthetic5", "synthetic16", "mea")
         for cut, seed in (((9.0, 9.0), 11), ((10.0, 8.0), 12))] + [("dipole", (9.0, 9.0), 13, True),
                                                                      ("synthetic5", (10.0, 8.0), 14, True)]
RECORD = {"force": 0.0, "torque": 0.0, "phi": 0.0, "field": 0.0, "allowed": [], "allowed_field": [], "skipped": 0,
          "run": 0}


@pytest.mark.parametrize("name,cut,seed,corner", CASES)
def test_the_restatement_against_central_differences_of_the_oracle(orc, water, name, cut, seed, corner):
    a = water
    sol = solutes(a)[name]
    S = sol.n_sites
    en = Energy(orc, a, sol, *cut)
    mol = placement(a, sol, seed, corner)
    q0 = np.asarray(sol.charge, dtype=float)
    su = ref.setup(a, orc, en.L, *cut)
    r = ref.replica(su, sol, mol, en.com, en.x, en.S_k(mol, q0))
    assert r["flags"] == 0 and r["n_counted"] > 0
    RECORD["run"] += 1
    if not ref.fd_safe(r, 2 * H):
        RECORD["skipped"] += 1
        assert 10 * RECORD["skipped"] <= len(CASES)
        return
    noise = EPS * sum(abs(t) for t in en.terms(mol, q0)) / (0.5 * H)

    def site_force(q, sites=range(S)):
        """(f [S, 3], its error [S, 3]) by central differences, the solute's charges being q."""
        f, err = np.zeros((S, 3)), np.zeros((S, 3))
        for k in sites:
            for d in range(3):
                def u(s, k=k, d=d):
                    m = mol.copy()
                    m[k, d] += s
                    return en(m, q)
                du, e = central(u, H)
                f[k, d], err[k, d] = -du, e
        return f, err

    f, err = site_force(q0)
    allowed = 10 * (err + noise)
    RECORD["allowed"] += [allowed.min(), allowed.max()]
    ratio = np.abs(f - r["site_force"]) / allowed
    RECORD["force"] = max(RECORD["force"], ratio.max())
    assert ratio.max() <= 1.0, (name, cut, f, r["site_force"], allowed)
    # the torque: the sites turned about c
    for axis in range(3):
        def u(s, axis=axis):
            m = mol.copy()
            m[:S] = mol[S] + r["d"] @ rotation(axis, s).T
            return en(m, q0)
        du, e = central(u, H)
        ratio = abs(-du - r["torque"][axis]) / (10 * (e + noise))
        RECORD["torque"] = max(RECORD["torque"], ratio)
        assert ratio <= 1.0, (name, cut, axis, -du, r["torque"][axis])
    # phi = dU / dq_a
    noise_q = EPS * sum(abs(t) for t in en.terms(mol, q0)) / (0.5 * DQ)
    for k in range(S):
        def u(s, k=k):
            q = q0.copy()
            q[k] += s
            return en(mol, q)
        du, e = central(u, DQ)
        ratio = abs(du - r["phi"][k]) / (10 * (e + noise_q))
        RECORD["phi"] = max(RECORD["phi"], ratio)
        assert ratio <= 1.0, (name, cut, k, du, r["phi"][k])
    # field[a] = d f_a / d q_a, exactly: f_a is linear in q_a
    for k in range(S):
        if not (S <= 5 or q0[k] == 0.0):
            continue
        qp, qm = q0.copy(), q0.copy()
        qp[k] += DQ_FIELD
        qm[k] -= DQ_FIELD
        (fp, ep), (fm, em) = site_force(qp, [k]), site_force(qm, [k])
        field = (fp[k] - fm[k]) / (2 * DQ_FIELD)
        allowed = 10 * ((ep[k] + em[k]) + 2 * noise) / (2 * DQ_FIELD)
        RECORD["allowed_field"] += [allowed.min(), allowed.max()]
        ratio = np.abs(field - r["field"][k]) / allowed
        RECORD["field"] = max(RECORD["field"], ratio.max())
        assert ratio.max() <= 1.0, (name, cut, k, field, r["field"][k], allowed)
        # ... and the intercept is the Lennard-Jones force
        mid = 0.5 * (fp[k] + fm[k]) - q0[k] * field
        assert np.all(np.abs(mid - r["site_lj"][k]) <= 10 * ((ep[k] + em[k]) + 2 * noise) * (1 + abs(q0[k]) / DQ_FIELD))
    # F and tau are the restated combinations of the site forces; recip + real + self = total
    assert np.allclose(r["site_force"], r["site_lj"] + q0[:, None] * r["field"], rtol=0, atol=1e-12 * r["A_site_force"].max())
    assert np.allclose(r["force"], r["site_force"].sum(0), rtol=0, atol=1e-12 * r["A_force"].max())
    assert np.allclose(r["torque"], np.cross(r["d"], r["site_force"]).sum(0), rtol=0, atol=1e-12 * r["A_torque"].max())
    assert np.allclose(r["field"], r["real"][:, :3] + r["recip"][:, :3], rtol=0, atol=1e-12 * r["A_field"].max())
    assert np.allclose(r["phi"], r["real"][:, 3] + r["recip"][:, 3] + r["self_phi"], rtol=0, atol=1e-12 * r["A_phi"].max())
    if RECORD["run"] == len(CASES):
        print(f"h = {H}: worst ratio site forces {RECORD['force']:.3g} torques {RECORD['torque']:.3g} phi {RECORD['phi']:.3g} "
              f"field {RECORD['field']:.3g}; allowed {min(RECORD['allowed']):.3g} .. {max(RECORD['allowed']):.3g}, "
              f"field {min(RECORD['allowed_field']):.3g} .. {max(RECORD['allowed_field']):.3g}; skipped {RECORD['skipped']}")


def test_the_self_term_is_ewald_self_differentiated(orc, water):
    sol = sr.dipole(water)
    en = Energy(orc, water, sol, 9.0, 9.0)
    su = ref.setup(water, orc, en.L, 9.0, 9.0)
    mol = placement(water, sol, 11)
    r = ref.replica(su, sol, mol, en.com, en.x, en.S_k(mol, sol.charge))
    # EwaldSelf is -kappa sum q^2 / sqrt(pi) factor: its q_a-derivative times q_a, summed, is twice it
    assert abs((r["self_phi"] * sol.charge).sum() - 2 * orc.ewald_self(en.ew, sol.charge)) < 1e-9


def test_an_atom_on_a_site_and_an_overlap_are_flagged(orc, water):
    sol = sr.cation(water)
    en = Energy(orc, water, sol, 9.0, 9.0)
    su = ref.setup(water, orc, en.L, 9.0, 9.0)
    S0 = np.zeros(su["cfac"].shape[0], dtype=complex)
    on = np.vstack([en.x[4], en.x[4]])                       # the site exactly on a hydrogen
    assert ref.replica(su, sol, on, en.com, en.x, S0)["flags"] == 2
    near = np.vstack([en.x[3] + [0.5, 0.2, 0.1], en.x[3] + [0.5, 0.2, 0.1]])   # r^2 = 0.3 from an oxygen
    assert ref.replica(su, sol, near, en.com, en.x, S0)["flags"] & 1


# ---- observables --------------------------------------------------------------------------------
def test_solute_mean_force_on_hand_made_numbers():
    f = np.array([[1.0, 2.0, 3.0], [3.0, 2.0, 1.0], [0.0, 0.0, 0.0], [2.0, 2.0, 5.0]])
    flags = np.array([0, 0, 1, 0], dtype=np.uint8)
    mean, err, n = obs.solute_mean_force(f, flags)
    assert n == 3 and np.allclose(mean, [2.0, 2.0, 3.0], rtol=0, atol=1e-15)
    assert np.allclose(err, np.std(f[[0, 1, 3]], axis=0, ddof=1) / np.sqrt(3), rtol=0, atol=1e-15)
    mean, err, n = obs.solute_mean_force(f[:1], flags[:1])
    assert n == 1 and np.array_equal(mean, f[0]) and np.all(np.isnan(err))
    with pytest.raises(ValueError):
        obs.solute_mean_force(f, flags[:3])


def test_pair_mean_force_projects_half_the_difference_on_the_axis():
    mol = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 4.0], [1.0, 1.0, 2.5]])   # a at z = 1, b at z = 4, then c
    sf = np.zeros((2, 2, 3))
    sf[0, 0], sf[0, 1] = [0.3, 0.0, -2.0], [0.0, 0.7, 4.0]
    sf[1, 0], sf[1, 1] = [0.0, 0.0, 1.0], [0.0, 0.0, 1.0]
    got = obs.pair_mean_force(sf, mol, 0, 1)
    assert np.allclose(got, [3.0, 0.0], rtol=0, atol=1e-15)               # > 0: the solvent pushes them apart
    assert np.allclose(obs.pair_mean_force(sf, mol, 1, 0), got, rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        obs.pair_mean_force(sf, mol, 0, 0)


def test_a_constant_mean_force_gives_a_linear_pmf():
    d = np.array([3.0, 4.0, 6.0, 7.5])
    w, w_err = obs.pmf_from_mean_force(d, np.full(4, 2.0), np.full(4, 0.1))
    assert np.allclose(w, 2.0 * (7.5 - d), rtol=0, atol=1e-14) and w[-1] == 0.0 and w_err[-1] == 0.0
    # the trapezoid's weights: the end points half an interval, the inner ones half of both
    assert np.allclose(w_err[0], 0.1 * np.sqrt(0.5 ** 2 + 1.5 ** 2 + 1.75 ** 2 + 0.75 ** 2), rtol=0, atol=1e-14)
    # the order of the separations does not matter
    w2, _ = obs.pmf_from_mean_force(d[::-1], np.full(4, 2.0), np.full(4, 0.1))
    assert np.allclose(w2[::-1], w, rtol=0, atol=1e-14)
    with pytest.raises(ValueError):
        obs.pmf_from_mean_force([1.0, 1.0], [0.0, 0.0], [0.0, 0.0])


def test_charging_with_phi_linear_in_lambda_gives_the_quadratic():
    q = np.array([0.5, -1.0])
    phi = np.array([[2.0, 1.0], [4.0, -1.0]])
    assert np.allclose(obs.charging_derivative(phi, q), [0.0, 3.0], rtol=0, atol=1e-15)
    lams = np.linspace(0.0, 1.0, 6)
    a, b = -300.0, 12.0                                       # <sum q phi>_lambda = a lambda + b
    dA, dA_err = obs.charging_free_energy(lams, a * lams + b, np.full(6, 0.5))
    assert abs(dA - (a / 2 + b)) < 1e-12
    wgt = np.full(6, 0.2)
    wgt[[0, -1]] = 0.1
    assert abs(dA_err - 0.5 * np.sqrt((wgt ** 2).sum())) < 1e-14
    with pytest.raises(ValueError):
        obs.charging_free_energy([0.0, 0.5, 0.5], [0, 0, 0], [0, 0, 0])
