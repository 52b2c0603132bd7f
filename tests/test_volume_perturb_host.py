"""CPU tests of the volume-perturbation definition (tests/volume_perturb_ref.py, on the oracle) and
of observables.pressure_from_volume_perturbation; and that the inputs the GPU tests use lie inside
the erfc table's domain and show the overlap they are built for."""
import math

import numpy as np
import pytest

import common
import volume_perturb_ref as ref
from metropolismontecarlo_amd import observables as obs

ALPHA = 5.6
T = 298.15
# the GPU tests' inputs (tests/test_gpu_volume_perturb.py imports them from here)
SCALES = (0.985, 0.999, 1.0, 1.001, 1.02)
RCUT = 10.0
EDGE_RCUT, EDGE_SCALES = 9.0, (0.95, 0.97, 1.0, 1.03)
OVL_SCALES = (0.95, 0.999, 1.0, 1.001, 1.02)
# ... and those of tests/test_gpu_volume_perturb_paths.py
CHUNK_N, CHUNK_SCALES = 16, (0.97,)                      # the first molecules of configuration 1
CONTACT_PAIR, CONTACT_R2 = (2, 5), 0.2                   # H of molecule 5 on H of molecule 2
MID_OVL_SCALES = (1.02, 1.0, 0.95, 1.001)                # the compressing scale at a middle index
OVL_PAIRS = {"tile0": (0, 1), "across": (3, 70), "ragged": (70, 90)}   # (100 molecules: tiles 64 + 36)
OVL_NOW_R2 = 0.48                                        # an overlap as stored
EIGHT_SCALES = (0.95, 0.97, 0.99, 0.999, 1.0, 1.001, 1.0 / 0.99, 1.03)
PREFIX_N = (1, 2, 63, 64, 65, 128, 129)
CUTOFFS = [(4, 8.0, 10.0, SCALES), (4, 10.0, 8.0, SCALES), (1, 7.5, 9.0, EDGE_SCALES), (1, 9.0, 7.5, EDGE_SCALES)]
LJ9_RCUT, LJ9_SCALES = 9.0, (0.9, 0.97, 1.0, 1.05)
LARGE_RCUT, LARGE_SCALES = 10.0, (0.99, 1.01)
NPT_SCALES = (0.99, 1.0, 1.01)
# the table's domain (csrc/mmc_fast.hpp: MMC_QQ_KAPPA_MAX, MMC_QQ_UMAX, MMC_QQ_XMAX)
KAPPA_MAX, UMAX, XMAX = 0.5, 256.0, 4.0


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def test_scale_one_gives_zero_and_weight_one(orc):
    a = common.nist_arrays(1, "unwrapped")
    p = ref.perturb(orc, a, (1.0, 1.01), ALPHA / a["box"], RCUT, T)
    assert np.array_equal(p["du"][0], np.zeros(4)) and p["w"][0] == 1.0 and not p["ovl"].any()
    assert np.all(p["du"][1] != 0.0) and np.isfinite(p["w"][1])
    # the restatement's rescale is the NPT tests' (L_new / L = f)
    b = ref.host_rescale(a, 1.01)
    assert b["box"] == 1.01 * a["box"] and np.array_equal(b["com"], a["com"] * 1.01)
    assert np.array_equal(b["coords"][4] - a["coords"][4], b["com"][1] - a["com"][1])


def test_ideal_gas_pressure_is_the_density(orc):
    """eps = q = 0: dU = 0, so beta P = N ln(V'/V) / dV exactly, -> rho as dv -> 0."""
    a = common.nist_arrays(1, "unwrapped")
    a = dict(a, eps=np.zeros_like(a["eps"]), charge=np.zeros_like(a["charge"]))
    n, L = a["com"].shape[0], a["box"]
    V = L ** 3
    dvs = np.array([40.0, -40.0, 0.4, -0.4])
    scales = [ref.scale_of_dv(L, dv) for dv in dvs]
    p = ref.perturb(orc, a, scales, ALPHA / L, RCUT, T)
    assert np.array_equal(p["du"], np.zeros((4, 4)))
    out = obs.pressure_from_volume_perturbation(p["w"][None, :], 1, dvs, T)
    want = n * np.log((V + dvs) / V) / dvs * T
    assert np.allclose(out["per_replica"][0], want, rtol=1e-9, atol=0)
    rho = n / V
    assert abs(out["per_replica"][0, 2] / T - rho) < 1e-4 * rho          # second order: dv / (2 V) = 2.5e-5
    assert abs(out["two_sided_pooled"][1] / T - rho) < 1e-8 * rho        # (dv / V)^2 / 3 = 8e-10


def test_dv_to_scale_conversion():
    L = 20.0
    for dv in (-300.0, -1.0, 0.0, 2.5, 400.0):
        f = ref.scale_of_dv(L, dv)
        assert f == ((L ** 3 + dv) / L ** 3) ** (1.0 / 3.0)
        assert abs((f * L) ** 3 - (L ** 3 + dv)) < 1e-9 * L ** 3
    assert ref.scale_of_dv(L, 0.0) == 1.0


def test_pooled_and_per_replica_estimators():
    rng = np.random.default_rng(5)
    dv = np.array([30.0, -30.0, 10.0])
    bs = rng.random((4, 3)) * 7 + 1.0
    n = 9
    out = obs.pressure_from_volume_perturbation(bs, n, dv, T)
    assert out["per_replica"].shape == (4, 3) and out["pooled"].shape == (3,)
    assert np.allclose(out["per_replica"], np.log(bs / n) * T / dv, rtol=1e-15)
    assert np.allclose(out["pooled"], np.log(bs.sum(0) / (4 * n)) * T / dv, rtol=1e-15)
    # the log of a mean is not the mean of the logs (Jensen): pooled differs unless the replicas agree
    assert not np.allclose(out["pooled"], out["per_replica"].mean(0))
    same = obs.pressure_from_volume_perturbation(np.tile(bs[:1], (4, 1)), n, dv, T)
    assert np.allclose(same["pooled"], same["per_replica"][0], rtol=1e-14)
    # two-sided: only +30 has its -30
    assert np.array_equal(out["two_sided_dv"], [30.0])
    assert np.allclose(out["two_sided_per_replica"][:, 0], (out["per_replica"][:, 0] + out["per_replica"][:, 1]) / 2)
    assert np.allclose(out["two_sided_pooled"], [(out["pooled"][0] + out["pooled"][1]) / 2])
    with pytest.raises(ValueError):
        obs.pressure_from_volume_perturbation(bs, n, dv[:2], T)
    with pytest.raises(ValueError):
        obs.pressure_from_volume_perturbation(bs, n, [1.0, 0.0, 2.0], T)


@pytest.mark.parametrize("config,rcut,scales", [(4, RCUT, SCALES), (1, EDGE_RCUT, EDGE_SCALES),
                                                (1, EDGE_RCUT, OVL_SCALES), (1, EDGE_RCUT, CHUNK_SCALES),
                                                (1, EDGE_RCUT, MID_OVL_SCALES), (1, EDGE_RCUT, EIGHT_SCALES)]
                         + [(1, EDGE_RCUT, (f,)) for f in EIGHT_SCALES]
                         + [(c, max(lj, qq), sc) for c, lj, qq, sc in CUTOFFS])
def test_gpu_inputs_stay_inside_the_table_domain(config, rcut, scales):
    L = common.nist_arrays(config, "unwrapped")["box"]
    l_min = min(scales) * L
    assert l_min >= 2 * rcut
    kappa = (ALPHA / L * L) / l_min
    assert kappa <= KAPPA_MAX and rcut * rcut + 100 <= UMAX
    assert kappa * math.sqrt(rcut * rcut + 100) <= XMAX


def test_the_constructed_overlap_shows_at_the_compressed_box_only(orc):
    a0 = common.nist_arrays(1, "unwrapped")
    a, dist = ref.overlap_case(a0)
    L = a["box"]
    h, o = a["coords"][4], a["coords"][0]
    assert abs(np.sum((h - o) ** 2) - 0.52) < 1e-12
    assert (math.sqrt(0.52) - 0.05 * dist) ** 2 < 0.45 and (math.sqrt(0.52) - 0.001 * dist) ** 2 > 0.51
    p = ref.perturb(orc, a, OVL_SCALES, ALPHA / L, EDGE_RCUT, T)
    assert list(p["ovl"]) == [True, False, False, False, False]
    assert p["w"][0] == 0.0 and p["w"][2] == 1.0 and np.all(np.isfinite(p["du"][1:]))
    # ... and the unmodified configuration overlaps nowhere
    assert not ref.perturb(orc, a0, OVL_SCALES, ALPHA / L, EDGE_RCUT, T)["ovl"].any()


def test_inputs_that_are_no_nist_configuration_stay_inside_the_table_domain():
    """The sibling of the test above for tests/test_gpu_volume_perturb_paths.py's other systems,
    by the rule the GPU tests themselves assert before a call (volume_perturb_ref.domain_ok), which
    is the arithmetic of the test above."""
    for L, rcut, scales in ((20.0, EDGE_RCUT, EDGE_SCALES), (30.0, RCUT, SCALES), (19.0, 9.0, (0.95, 1.0))):
        l_min = min(scales) * L
        kappa = ALPHA / l_min
        want = (l_min >= 2 * rcut and kappa <= KAPPA_MAX and rcut * rcut + 100 <= UMAX
                and kappa * math.sqrt(rcut * rcut + 100) <= XMAX)
        assert ref.domain_ok(L, rcut, scales, ALPHA) == want
    assert not ref.domain_ok(20.0, EDGE_RCUT, (0.89,)) and not ref.domain_ok(15.73, 7.0, (0.97,))
    # prefixes of the dense lattice of 300, in its box
    a = ref.dense_prefix(max(PREFIX_N))
    assert abs(a["box"] - (300 / 0.033101144) ** (1 / 3)) < 1e-9
    assert ref.domain_ok(a["box"], EDGE_RCUT, EDGE_SCALES)
    # nine LJ pairs
    assert ref.domain_ok(ref.lj9_system()["box"], LJ9_RCUT, LJ9_SCALES)
    # the largest systems one workgroup's LDS can hold: 56 bytes per atom beside 2 x 352 x 8 of S(k),
    # for every LDS size from 64 to 160 KiB, and the system one molecule too large (refused, but for
    # the LDS rule alone)
    from test_gpu_batch import _dense_water
    for lds in (64 << 10, 160 << 10):
        n = ((lds - 256) // 8 - 2 * 352) // 7 // 3
        for n_mol in (n, n + 1, n + 60):
            assert ref.domain_ok((n_mol / 0.033101144) ** (1 / 3), LARGE_RCUT, LARGE_SCALES), n_mol
    assert abs(_dense_water(355)["box"] - (355 / 0.033101144) ** (1 / 3)) < 1e-9
    # after an accepted volume move to 1.01 V, and after an NPT chain that keeps within 2 % of L
    L = common.nist_arrays(1, "unwrapped")["box"]
    assert ref.domain_ok(1.01 ** (1 / 3) * L, EDGE_RCUT, EDGE_SCALES)
    assert ref.domain_ok(0.98 * L, EDGE_RCUT, NPT_SCALES) and ref.domain_ok(1.02 * L, EDGE_RCUT, NPT_SCALES)


def test_the_oracle_takes_the_tiny_prefixes(orc):
    """One and two molecules: no pair (or one), the reciprocal and self parts alone change."""
    for n in (1, 2):
        a = ref.dense_prefix(n)
        p = ref.perturb(orc, a, EDGE_SCALES, ALPHA / a["box"], EDGE_RCUT, T)
        assert np.all(np.isfinite(p["du"])) and not p["ovl"].any() and np.all(p["du"][2] == 0.0)
        assert np.all(p["du"][[0, 1, 3], 2:] != 0.0)
    assert np.array_equal(ref.prefix(a, 1)["coords"], a["coords"][:3])


def test_separate_cutoffs_reach_the_reference(orc):
    """parts_at with two cutoffs: LJ follows the first, the real part the second, and the default is
    the single-cutoff call."""
    a = common.nist_arrays(1, "unwrapped")
    k = ALPHA / a["box"]
    both, _ = ref.parts_at(orc, a, 0.97, k, 9.0)
    same, _ = ref.parts_at(orc, a, 0.97, k, 9.0, 9.0)
    assert np.array_equal(both, same)
    lj, _ = ref.parts_at(orc, a, 0.97, k, 7.5, 9.0)
    qq, _ = ref.parts_at(orc, a, 0.97, k, 9.0, 7.5)
    assert lj[0] != both[0] and lj[1] == both[1] and qq[0] == both[0] and qq[1] != both[1]
    assert np.array_equal(lj[2:], both[2:]) and np.array_equal(qq[2:], both[2:])
    p = ref.perturb(orc, a, EDGE_SCALES, k, 7.5, T, qq_rcut=9.0)
    assert np.array_equal(p["base"], ref.parts_at(orc, a, 1.0, k, 7.5, 9.0)[0])


def test_the_close_like_charge_contact(orc):
    """Two hydrogens at r^2 = 0.2: below the erfc table's first node (0.25) at f <= 1 and above it
    at 1.03, no opposite charges anywhere near, no overlap, a finite real part -- and a pair term
    that knows its box's kappa: with the batch's kappa in place of kappa_k = alpha / (f L) the real
    part of the compressed boxes moves by 1e-4 of itself, 1e5 times the GPU tests' tolerance."""
    from metropolismontecarlo_amd import structs
    a0 = common.nist_arrays(1, "unwrapped")
    i, j = CONTACT_PAIR
    a, dist = ref.contact_case(a0, i, j, CONTACT_R2)
    L = a["box"]
    qh = float(a["charge"][3 * i + 1])
    assert qh > 0 and a["charge"][3 * j + 1] == qh
    r2 = [ref.pair_r2(a, f, i, 1, j, 1) for f in EDGE_SCALES]
    assert abs(r2[2] - CONTACT_R2) < 1e-12 and EDGE_SCALES[2] == 1.0
    assert r2[0] < r2[1] < 0.25 and EDGE_SCALES[0] != 1.0 and EDGE_SCALES[1] != 1.0     # the series branch
    assert r2[3] > 0.25                                                              # ... and back on the table
    for f, x in zip(EDGE_SCALES, r2):
        assert abs(math.sqrt(x) - (math.sqrt(CONTACT_R2) + (f - 1.0) * dist)) < 1e-12
        assert ref.min_r2_opposite(a, f) > 0.5
    assert ref.min_r2_opposite(a, 1.0) > 0.5
    p = ref.perturb(orc, a, EDGE_SCALES, ALPHA / L, EDGE_RCUT, T)
    assert not p["ovl"].any() and np.all(np.isfinite(p["du"])) and np.all(np.isfinite(p["base"]))
    k0 = ALPHA / L
    for k, f in enumerate(EDGE_SCALES[:2]):
        kk, r = ALPHA / (f * L), math.sqrt(r2[k])
        real = p["base"][1] + p["du"][k, 1]
        wrong = structs.factor * qh * qh * (math.erfc(k0 * r) - math.erfc(kk * r)) / r
        assert abs(kk - k0) > 0.008 and abs(wrong) > 1e-4 * abs(real), (f, wrong, real)


@pytest.mark.parametrize("where", sorted(OVL_PAIRS))
def test_the_constructed_overlaps_show_at_the_middle_scale_only(orc, where):
    a0 = common.nist_arrays(1, "unwrapped")
    i, j = OVL_PAIRS[where]
    assert {"tile0": i < j < 64, "across": i < 64 <= j, "ragged": 64 <= i < j < 100}[where]
    a, dist = ref.overlap_case(a0, i, j)
    assert abs(ref.pair_r2(a, 1.0, i, 0, j, 1) - 0.52) < 1e-12
    p = ref.perturb(orc, a, MID_OVL_SCALES, ALPHA / a["box"], EDGE_RCUT, T)
    assert list(p["ovl"]) == [False, False, True, False]
    assert list(p["w"] == 0.0) == [False, False, True, False] and p["w"][1] == 1.0
    # the pair itself is the only one below 0.5, at that scale only
    for f in MID_OVL_SCALES:
        assert (ref.min_r2_opposite(a, f) < 0.5) == (f == 0.95)
    assert abs(ref.min_r2_opposite(a, 0.95) - ref.pair_r2(a, 0.95, i, 0, j, 1)) < 1e-12
    assert not ref.perturb(orc, a0, MID_OVL_SCALES, ALPHA / a["box"], EDGE_RCUT, T)["ovl"].any()


def test_the_overlap_that_is_there_already(orc):
    """r^2 = 0.48 as stored: every test box is flagged, also the expanded one (1.02) whose own pair
    distance is beyond 0.5; the other three parts stay finite."""
    a0 = common.nist_arrays(1, "unwrapped")
    a, dist = ref.overlap_case(a0, 0, 1, r2=OVL_NOW_R2)
    assert abs(ref.pair_r2(a, 1.0, 0, 0, 1, 1) - OVL_NOW_R2) < 1e-12
    assert ref.min_r2_opposite(a, 1.02) > 0.5
    p = ref.perturb(orc, a, MID_OVL_SCALES, ALPHA / a["box"], EDGE_RCUT, T)
    assert p["ovl"].all() and np.all(p["w"] == 0.0)
    assert np.all(np.isfinite(p["base"][[0, 2, 3]])) and np.all(np.isfinite(p["du"][:, [0, 2, 3]]))


def test_the_other_systems_overlap_nowhere(orc):
    for a, rcut, scales in ((ref.lj9_system(), LJ9_RCUT, LJ9_SCALES),
                            (ref.dense_prefix(129), EDGE_RCUT, EDGE_SCALES),
                            (ref.prefix(common.nist_arrays(1, "unwrapped"), CHUNK_N), EDGE_RCUT, CHUNK_SCALES)):
        p = ref.perturb(orc, a, scales, ALPHA / a["box"], rcut, T)
        assert not p["ovl"].any() and np.all(np.isfinite(p["du"])), rcut
    a = ref.prefix(common.nist_arrays(1, "unwrapped"), CHUNK_N)
    st = ref.shifted_states(a, 5)
    for k, s in enumerate(st):
        p = ref.perturb(orc, s, CHUNK_SCALES, ALPHA / a["box"], EDGE_RCUT, T)
        assert not p["ovl"].any() and np.all(np.isfinite(p["du"]))
        assert all(not np.array_equal(s["com"], o["com"]) for o in st[:k] + [a])
    # eight scales: distinct, 1.0 among them, one pair reciprocal around 1
    assert len(set(EIGHT_SCALES)) == 8 and 1.0 in EIGHT_SCALES and EIGHT_SCALES[2] * EIGHT_SCALES[6] == 1.0
