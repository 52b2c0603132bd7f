"""CPU tests of the boundary of mmc_batch_cavity and mmc_batch_cavity_at: declared with the agreed
prototypes, exported, bound with matching ctypes, and loud on a NULL batch and on every argument
that can be refused without a device."""
import ctypes as C
import re

import pytest

import boundary
from metropolismontecarlo_amd import _lib

PROTOTYPES = {
    "mmc_batch_cavity": (
        "int32_t mmc_batch_cavity(mmc_batch *b, int64_t n_probe, uint64_t seed, int64_t draw0, int32_t site, "
        "int32_t n_radii, const double *radii, int32_t n_cap, int32_t nn_bins, double nn_max, int32_t per_replica, "
        "uint64_t *occ_hist, uint64_t *occ_mom, uint64_t *nn_hist, double *points_out, int32_t *count_out, "
        "double *nn_r2_out, int32_t *nn_idx_out);"),
    "mmc_batch_cavity_at": (
        "int32_t mmc_batch_cavity_at(mmc_batch *b, int64_t n_probe, const double *points_in, int32_t site, "
        "int32_t n_radii, const double *radii, int32_t n_cap, int32_t nn_bins, double nn_max, int32_t per_replica, "
        "uint64_t *occ_hist, uint64_t *occ_mom, uint64_t *nn_hist, int32_t *count_out, double *nn_r2_out, "
        "int32_t *nn_idx_out);"),
}


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_symbols_are_declared_exported_and_bound_with_the_header_prototype(name):
    """(Exported and bound with these types: tests/test_abi.py, for every function of the header.)"""
    assert boundary.prototype_text(name) == PROTOTYPES[name]


def test_the_constants_of_the_header():
    code = boundary.header_code()
    assert re.search(r"#define\s+MMC_SLOT_CAVITY\s+MMC_SLOT_WIDOM\b", code)
    for name, value in (("MMC_CAVITY_MAX_RADII", 8), ("MMC_CAVITY_MAX_CAP", 255), ("MMC_CAVITY_MAX_BINS", 4096)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), code), name


def call(at=False, b=None, n_probe=10, site=0, radii=(1.0, 2.0), n_radii=None, n_cap=4, nn_bins=16, nn_max=5.0,
         outputs=(True, True, True), points=True):
    """One call with sentinel outputs, which must come back untouched.  Returns (status, message)."""
    K = len(radii) if radii is not None else 0
    n_radii = K if n_radii is None else n_radii
    rad = (C.c_double * max(K, 1))(*(radii or ())) if radii is not None else None
    oh = (C.c_uint64 * 4096)(*([77] * 4096))
    om = (C.c_uint64 * 16)(*([77] * 16))
    nh = (C.c_uint64 * 4100)(*([77] * 4100))
    pts = (C.c_double * 30)(*([7.5] * 30))
    cnt = (C.c_int32 * 80)(*([-5] * 80))
    r2 = (C.c_double * 10)(*([7.5] * 10))
    ix = (C.c_int32 * 10)(*([-5] * 10))
    L = _lib.lib()
    common = (site, n_radii, rad, n_cap, nn_bins, nn_max, 0, oh if outputs[0] else None, om if outputs[1] else None,
              nh if outputs[2] else None)
    if at:
        st = L.mmc_batch_cavity_at(b, n_probe, pts if points else None, *common, cnt, r2, ix)
    else:
        st = L.mmc_batch_cavity(b, n_probe, 1234, 0, *common, pts, cnt, r2, ix)
    assert all(v == 77 for v in oh) and all(v == 77 for v in om) and all(v == 77 for v in nh)
    assert all(v == 7.5 for v in pts) and all(v == -5 for v in cnt) and all(v == 7.5 for v in r2)
    assert all(v == -5 for v in ix)
    msg = L.mmc_last_error()
    return st, (msg.decode() if msg else "")


@pytest.mark.parametrize("at", [False, True])
def test_a_null_batch_fails_loudly(at):
    st, msg = call(at)
    assert st == _lib.MMC_ERR_ARG and "NULL" in msg
    with pytest.raises(_lib.MMCError, match="MMC_ERR_ARG"):
        _lib.check(st)


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("at", [False, True])
@pytest.mark.parametrize("kw,word", [
    (dict(n_probe=0), "n_probe"), (dict(n_probe=-3), "n_probe"), (dict(n_probe=(1 << 20) + 1), "n_probe"),
    (dict(site=3), "site"), (dict(site=-2), "site"),
    (dict(n_radii=0), "n_radii"), (dict(n_radii=-1), "n_radii"), (dict(radii=(1.0,) * 9), "n_radii"),
    (dict(radii=None, n_radii=2), "radii"),
    (dict(radii=(NAN,)), "radii"), (dict(radii=(1.0, INF)), "radii"), (dict(radii=(0.0, 1.0)), "radii"),
    (dict(radii=(-1.0,)), "radii"), (dict(radii=(1.0, 1.0)), "radii"), (dict(radii=(2.0, 1.0)), "radii"),
    (dict(n_cap=0), "n_cap"), (dict(n_cap=-1), "n_cap"), (dict(n_cap=256), "n_cap"),
    (dict(nn_bins=0), "nn_bins"), (dict(nn_bins=-1), "nn_bins"), (dict(nn_bins=4097), "nn_bins"),
    (dict(nn_max=NAN), "nn_max"), (dict(nn_max=INF), "nn_max"), (dict(nn_max=0.0), "nn_max"),
    (dict(nn_max=-5.0), "nn_max"),
    (dict(outputs=(False, False, False)), "at least one"),
])
def test_arguments_refused_without_a_device(at, kw, word):
    """These are refused before the batch is looked at: the message names the argument, not the
    NULL batch, and nothing is written."""
    st, msg = call(at, **kw)
    assert st == _lib.MMC_ERR_ARG
    assert word in msg and "batch is NULL" not in msg, msg


def test_null_points_are_refused_without_a_device():
    st, msg = call(True, points=False)
    assert st == _lib.MMC_ERR_ARG and "points_in" in msg and "batch is NULL" not in msg, msg


def test_the_bin_arguments_are_ignored_without_nn_hist():
    """nn_bins and nn_max are only looked at when nn_hist is given: the call gets as far as the batch."""
    for at in (False, True):
        st, msg = call(at, nn_bins=-7, nn_max=NAN, outputs=(True, True, False))
        assert st == _lib.MMC_ERR_ARG and "batch is NULL" in msg, msg
