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
                                                (1, EDGE_RCUT, OVL_SCALES)])
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
