"""CPU tests of mmc_batch_voronoi's boundary: declared with the agreed prototype, exported, bound
with matching ctypes, carried by the Julia module and the Python class, and loud on a NULL batch
and on every argument that can be refused without a device -- with the outputs untouched."""
import ctypes as C

import pytest

import boundary
from metropolismontecarlo_amd import _lib

NAME = "mmc_batch_voronoi"
PROTOTYPE = ("int32_t mmc_batch_voronoi(mmc_batch *b, double r_list, double area_min, int32_t v_bins, double v_max, "
             "int32_t eta_bins, double eta_max, int32_t r_bins, int32_t per_replica, "
             "uint64_t *vol_hist, uint64_t *eta_hist, uint64_t *face_hist, uint64_t *side_hist, uint64_t *nbr_hist, "
             "uint64_t *flagged, double *sums, "
             "double *vol_out, double *area_out, int32_t *faces_out, int32_t *nbr_out, double *face_area_out);")
INF, NAN = float("inf"), float("nan")


def test_symbol_is_declared_exported_and_bound_with_the_header_prototype():
    """(Exported and bound with these types: tests/test_abi.py, for every function of the header.)"""
    assert boundary.prototype_text(NAME) == PROTOTYPE
    assert len(boundary.header_prototypes()[NAME][1]) == 21


def test_the_header_states_the_constants_the_rule_and_the_limits():
    text = boundary.header_text()
    for word in ("#define MMC_VORONOI_CAP      64", "#define MMC_VORONOI_MAXV     16", "MMC_VORONOI_PRUNE, PRUNE = 1 + 2^-20",
                 "w = e(p_j) / (e(p_j) - e(q))", "K = 36.0 x 3.141592653589793", "biased low", "voronoi_prune"):
        assert word in text, word


def test_the_julia_binding_and_the_python_method_carry_it():
    import inspect
    from metropolismontecarlo_amd import observables as obs
    from metropolismontecarlo_amd.device import Batch
    jl = boundary.julia_text()
    assert ":mmc_batch_voronoi" in jl and "function voronoi(" in jl
    sig = inspect.signature(Batch.voronoi)
    assert [(k, p.default) for k, p in sig.parameters.items()][1:] == [
        ("r_list", 7.0), ("area_min", 0.0), ("v_bins", 200), ("v_max", 80.0), ("eta_bins", 200), ("eta_max", 3.0),
        ("r_bins", 280), ("per_replica", False), ("details", False), ("out", None)]
    for name in ("voronoi_volume_distribution", "asphericity_distribution", "voronoi_coordination",
                 "face_side_fractions", "voronoi_neighbour_gr", "voronoi_means", "volume_fluctuation"):
        assert callable(getattr(obs, name)), name


SIZE = 1025
N_OUT = 12


def call(b=None, r_list=7.0, area_min=0.0, v_bins=200, v_max=80.0, eta_bins=200, eta_max=3.0, r_bins=280,
         outputs=(True,) * N_OUT):
    u64 = [(C.c_uint64 * SIZE)(*([77] * SIZE)) for _ in range(6)]           # five histograms, flagged
    dbl = [(C.c_double * SIZE)(*([7.5] * SIZE)) for _ in range(4)]          # sums, vol, area, face_area
    i32 = [(C.c_int32 * SIZE)(*([-5] * SIZE)) for _ in range(2)]            # faces, nbr
    args = u64 + [dbl[0], dbl[1], dbl[2], i32[0], i32[1], dbl[3]]
    st = _lib.lib().mmc_batch_voronoi(b, r_list, area_min, v_bins, v_max, eta_bins, eta_max, r_bins, 0,
                                      *[a if on else None for a, on in zip(args, outputs)])
    assert all(v == 77 for h in u64 for v in h) and all(v == 7.5 for h in dbl for v in h)
    assert all(v == -5 for h in i32 for v in h)
    msg = _lib.lib().mmc_last_error()
    return st, (msg.decode() if msg else "")


def test_a_null_batch_fails_loudly():
    st, msg = call()
    assert st == _lib.MMC_ERR_ARG and "NULL" in msg
    with pytest.raises(_lib.MMCError, match="MMC_ERR_ARG"):
        _lib.check(st)
    # the largest bins, area_min > 0 and a single output pass the argument checks too
    st, msg = call(v_bins=1024, eta_bins=1024, r_bins=1024, area_min=1e-6)
    assert st == _lib.MMC_ERR_ARG and "NULL" in msg
    for only in range(N_OUT):
        st, msg = call(outputs=tuple(k == only for k in range(N_OUT)))
        assert st == _lib.MMC_ERR_ARG and "batch is NULL" in msg, only


@pytest.mark.parametrize("kw,word", [
    (dict(r_list=NAN), "r_list"), (dict(r_list=INF), "r_list"), (dict(r_list=0.0), "r_list"), (dict(r_list=-7.0), "r_list"),
    (dict(area_min=-1e-9), "area_min"), (dict(area_min=NAN), "area_min"), (dict(area_min=INF), "area_min"),
    (dict(v_bins=0), "v_bins"), (dict(v_bins=1025), "v_bins"), (dict(v_bins=-3), "v_bins"),
    (dict(v_max=0.0), "v_max"), (dict(v_max=-80.0), "v_max"), (dict(v_max=NAN), "v_max"), (dict(v_max=INF), "v_max"),
    (dict(eta_bins=0), "eta_bins"), (dict(eta_bins=1025), "eta_bins"),
    (dict(eta_max=1.0), "eta_max"), (dict(eta_max=0.5), "eta_max"), (dict(eta_max=NAN), "eta_max"),
    (dict(eta_max=INF), "eta_max"),
    (dict(r_bins=0), "r_bins"), (dict(r_bins=1025), "r_bins"),
    (dict(outputs=(False,) * N_OUT), "at least one"),
])
def test_arguments_refused_without_a_device(kw, word):
    """These are refused before the batch is looked at: the message names the argument, not the
    NULL batch, and nothing is written."""
    st, msg = call(**kw)
    assert st == _lib.MMC_ERR_ARG
    assert word in msg and "batch is NULL" not in msg, msg
