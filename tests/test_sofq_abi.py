"""CPU tests of mmc_batch_structure_factor's boundary: declared with the agreed prototype, exported,
bound with matching ctypes, loud on a NULL batch and on every argument that can be refused without a
device, and the Python wrapper's own check of `out`."""
import ctypes as C

import numpy as np
import pytest

import boundary
from boundary import header_define
from common import fake_batch
from metropolismontecarlo_amd import _lib

NAME = "mmc_batch_structure_factor"
PROTOTYPE = ("int32_t mmc_batch_structure_factor(mmc_batch *b, int32_t n_max, int32_t per_replica, "
             "int32_t *count, int64_t *sq, double *sq_sum);")
SENTINEL = -0x0123456789abcdef


def test_symbol_is_declared_exported_and_bound_with_the_header_prototype():
    """(Exported and bound with these types: tests/test_abi.py, for every function of the header.)"""
    assert boundary.prototype_text(NAME) == PROTOTYPE


def test_the_header_states_the_definition_and_its_constants():
    src = boundary.header_text()
    sec = src[src.index("Partial structure factors"):src.index("int32_t mmc_batch_structure_factor")]
    assert src.index("Orientational pair correlations") < src.index("Partial structure factors") < src.index("Local order")
    for cite in ("Ewald/ewalds.jl:538-604", ":575-585", "0 < s = nx^2 + ny^2 + nz^2 <= n_max^2", "q = 2 pi n / L",
                 "r_3(s)", "nx = ny = 0 and nz > 0", "rho(-n) = conj rho(n)", "no imaging", "sincos_moderate",
                 "repeated c_mul", "conjugation", "(x y) z", "l, l + 64", "wave_sum", "one wave computes",
                 "(0,0) (0,1) (0,2) (1,1) (1,2) (2,2)", "rho_a.re rho_b.re + rho_a.im rho_b.im", "unfused",
                 "ties to even", "holds the cross term once", "S_aa -> 1", "2^54", "ascending",
                 "sq[R][6][n_max^2 + 1]", "MMC_ERR_STATE", "MMC_ERR_UNSUPPORTED", "MMC_SOFQ_MAX_MOL",
                 "per-replica boxes", "tests/sofq_ref.py", "left untouched"):
        assert cite in sec, cite
    assert int(header_define("MMC_SOFQ_MAX_N")) == 32
    assert int(header_define("MMC_SOFQ_MAX_MOL")) == 1024
    assert float(header_define("MMC_SOFQ_SCALE")) == 2.0 ** 24
    # the phases of MMC_SOFQ_MAX_MOL molecules, 48 bytes per atom, in the 160 KB of a compute unit's LDS
    assert 48 * 3 * 1024 <= 160 * 1024 - 64


def test_the_julia_binding_calls_it():
    assert NAME in boundary.julia_bound()


def call(b=None, n_max=4, per_replica=0, count=True, sq=None, sq_sum=None):
    """sq / sq_sum default to what per_replica selects."""
    sq = bool(per_replica) if sq is None else sq
    sq_sum = (not per_replica) if sq_sum is None else sq_sum
    c = (C.c_int32 * 64)(*([-7] * 64))
    q = (C.c_int64 * 256)(*([SENTINEL] * 256))
    d = (C.c_double * 256)(*([-1.25] * 256))
    st = _lib.lib().mmc_batch_structure_factor(b, n_max, per_replica, c if count else None, q if sq else None,
                                               d if sq_sum else None)
    assert all(v == -7 for v in c) and all(v == SENTINEL for v in q) and all(v == -1.25 for v in d)
    msg = _lib.lib().mmc_last_error()
    return st, (msg.decode() if msg else "")


def test_a_null_batch_fails_loudly():
    for kw in (dict(), dict(per_replica=1), dict(n_max=32, count=False), dict(n_max=1, per_replica=5)):
        st, msg = call(**kw)
        assert st == _lib.MMC_ERR_ARG and "batch is NULL" in msg, kw
    with pytest.raises(_lib.MMCError, match="MMC_ERR_ARG"):
        _lib.check(st)


@pytest.mark.parametrize("kw,word", [
    (dict(n_max=0), "n_max"), (dict(n_max=-1), "n_max"), (dict(n_max=33), "n_max"), (dict(n_max=2 ** 31 - 1), "n_max"),
    (dict(n_max=0, per_replica=1), "n_max"),
    (dict(per_replica=0, sq_sum=False), "sq_sum is a NULL"), (dict(per_replica=1, sq=False), "sq is a NULL"),
    (dict(per_replica=0, sq=True), "takes no sq"), (dict(per_replica=1, sq_sum=True), "takes no sq_sum"),
    (dict(per_replica=0, sq=False, sq_sum=False), "NULL"), (dict(per_replica=1, sq=False, sq_sum=False), "NULL"),
])
def test_arguments_refused_without_a_device(kw, word):
    """These are refused before the batch is looked at: the message names the argument, not the NULL
    batch, and nothing is written."""
    st, msg = call(**kw)
    assert st == _lib.MMC_ERR_ARG
    assert word in msg and "batch is NULL" not in msg, msg


# (device.Batch.structure_factor's own check of `out` runs before the library is called.)
@pytest.mark.parametrize("kw", [
    dict(out=np.zeros((6, 10), dtype=np.int64)), dict(out=np.zeros((6, 9), dtype=np.float64)),
    dict(out=np.zeros((2, 6, 10), dtype=np.float64)), dict(out=np.zeros((6, 20), dtype=np.float64)[:, ::2]),
    dict(out=[[0.0] * 10] * 6), dict(out=np.zeros((6, 10), dtype=np.float64), per_replica=True),
    dict(out=np.zeros((2, 6, 10), dtype=np.float64), per_replica=True),
    dict(out=np.zeros((2, 6, 10), dtype=np.uint64), per_replica=True),
])
def test_the_wrapper_checks_its_arguments(kw):
    with pytest.raises(ValueError):
        fake_batch("structure_factor").structure_factor(3, **kw)
    with pytest.raises(AssertionError, match="the library was reached"):
        fake_batch("structure_factor").structure_factor(3, out=np.zeros((6, 10), dtype=np.float64))
    with pytest.raises(AssertionError, match="the library was reached"):
        fake_batch("structure_factor").structure_factor(3, per_replica=True, out=np.zeros((2, 6, 10), dtype=np.int64))
