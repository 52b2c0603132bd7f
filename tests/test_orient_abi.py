"""CPU tests of mmc_batch_orient_corr's boundary: declared with the agreed prototype, exported, bound
with matching ctypes, loud on a NULL batch and on every argument that can be refused without a
device, and the Python wrapper's own check of `out`."""
import ctypes as C

import numpy as np
import pytest

import boundary
from boundary import header_define
from common import fake_batch
from metropolismontecarlo_amd import _lib

NAME = "mmc_batch_orient_corr"
PROTOTYPE = ("int32_t mmc_batch_orient_corr(mmc_batch *b, int32_t numbins, double r_max, int32_t per_replica, "
             "int64_t *hist);")
SENTINEL = -0x0123456789abcdef


def test_symbol_is_declared_exported_and_bound_with_the_header_prototype():
    """(Exported and bound with these types: tests/test_abi.py, for every function of the header.)"""
    assert boundary.prototype_text(NAME) == PROTOTYPE


def test_the_header_states_the_definition_and_its_constants():
    src = boundary.header_text()
    sec = src[src.index("Orientational pair correlations"):src.index("int32_t mmc_batch_orient_corr")]
    assert src.index("Structure observables") < src.index("Orientational pair correlations") < src.index("Local order")
    for cite in ("row (0,0) of mmc_batch_rdf_sites", "gr.jl:75-80", "mmc_batch_dipoles", "u = mu / sqrt(n^2)",
                 "u = 0 when n^2 is 0 or not finite", "p2 = 1.5 c^2 - 0.5", "hd = 3 (u_i . d)(u_j . d) / r^2 - c",
                 "hd = 0 when r^2 = 0", "ties to even", "slot numbins + 1", "rows 2 and 3 are 0", "2^-31",
                 "hist[R][4][numbins + 2]", "MMC_ERR_STATE", "MMC_ORIENT_MAX_BINS", "2^21", "tests/orient_ref.py"):
        assert cite in sec, cite
    assert float(header_define("MMC_ORIENT_SCALE")) == 2.0 ** 30
    # what one wave fits: thresholds (8 bytes) and four 64-bit rows (32 bytes) per slot in 64 KB
    max_bins = int(header_define("MMC_ORIENT_MAX_BINS"))
    assert 40 * (max_bins + 2) <= 65536 < 40 * (max_bins + 3)


def test_the_julia_binding_calls_it():
    assert NAME in boundary.julia_bound()


def call(b=None, numbins=10, r_max=0.0, per_replica=0, hist=True):
    h = (C.c_int64 * 64)(*([SENTINEL] * 64))
    st = _lib.lib().mmc_batch_orient_corr(b, numbins, r_max, per_replica, h if hist else None)
    assert all(v == SENTINEL for v in h)
    msg = _lib.lib().mmc_last_error()
    return st, (msg.decode() if msg else "")


def test_a_null_batch_fails_loudly():
    st, msg = call()
    assert st == _lib.MMC_ERR_ARG and "batch is NULL" in msg
    with pytest.raises(_lib.MMCError, match="MMC_ERR_ARG"):
        _lib.check(st)
    st, msg = call(numbins=int(header_define("MMC_ORIENT_MAX_BINS")), r_max=3.0, per_replica=1)
    assert st == _lib.MMC_ERR_ARG and "batch is NULL" in msg


@pytest.mark.parametrize("kw,word", [
    (dict(hist=False), "NULL out pointer"),
    (dict(numbins=0), "numbins"), (dict(numbins=-7), "numbins"),
    (dict(numbins=1637), "numbins"), (dict(numbins=2 ** 31 - 1), "numbins"),
    (dict(r_max=float("nan")), "r_max"), (dict(r_max=float("inf")), "r_max"), (dict(r_max=-float("inf")), "r_max"),
])
def test_arguments_refused_without_a_device(kw, word):
    """These are refused before the batch is looked at: the message names the argument, not the NULL
    batch, and nothing is written.  (An r_max against the boxes needs the batch:
    tests/test_gpu_orient.py.)"""
    assert int(header_define("MMC_ORIENT_MAX_BINS")) == 1636
    st, msg = call(**kw)
    assert st == _lib.MMC_ERR_ARG
    assert word in msg and "batch is NULL" not in msg, msg


# (device.Batch.orient_corr's own check of `out` runs before the library is called.)
@pytest.mark.parametrize("kw", [
    dict(out=np.zeros((4, 12), dtype=np.uint64)), dict(out=np.zeros((4, 11), dtype=np.int64)),
    dict(out=np.zeros((2, 4, 12), dtype=np.int64)), dict(out=np.zeros((4, 24), dtype=np.int64)[:, ::2]),
    dict(out=[[0] * 12] * 4), dict(out=np.zeros((4, 12), dtype=np.int64), per_replica=True),
])
def test_the_wrapper_checks_its_arguments(kw):
    with pytest.raises(ValueError):
        fake_batch("orient_corr").orient_corr(10, **kw)
    with pytest.raises(AssertionError, match="the library was reached"):
        fake_batch("orient_corr").orient_corr(10, out=np.zeros((4, 12), dtype=np.int64))
