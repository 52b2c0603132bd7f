"""CPU tests of mmc_batch_local_order's boundary: declared with the agreed prototype, exported,
bound with matching ctypes, and loud on a NULL batch and on every argument that can be refused
without a device."""
import ctypes as C
import math

import pytest

import boundary
from metropolismontecarlo_amd import _lib

NAME = "mmc_batch_local_order"
PROTOTYPE = ("int32_t mmc_batch_local_order(mmc_batch *b, double r_hb, double cos_hb, int32_t q_bins, "
             "int32_t per_replica, uint64_t *hb_hist, uint64_t *q_hist, double *q_sum, int32_t *nbr_out, "
             "double *q_out, uint8_t *hb_out);")


def test_symbol_is_declared_exported_and_bound_with_the_header_prototype():
    """(Exported and bound with these types: tests/test_abi.py, for every function of the header.)"""
    assert boundary.prototype_text(NAME) == PROTOTYPE


def call(b=None, r_hb=3.5, cos_hb=math.cos(math.radians(30.0)), q_bins=400, outputs=(True, True, True)):
    hb = (C.c_uint64 * 27)(*([77] * 27))
    qh = (C.c_uint64 * 4096)(*([77] * 4096))
    qs = (C.c_double * 2)(7.5, 7.5)
    st = _lib.lib().mmc_batch_local_order(b, r_hb, cos_hb, q_bins, 0, hb if outputs[0] else None,
                                          qh if outputs[1] else None, qs if outputs[2] else None,
                                          None, None, None)
    assert all(v == 77 for v in hb) and all(v == 77 for v in qh) and list(qs) == [7.5, 7.5]
    msg = _lib.lib().mmc_last_error()
    return st, (msg.decode() if msg else "")


def test_a_null_batch_fails_loudly():
    st, msg = call()
    assert st == _lib.MMC_ERR_ARG and "NULL" in msg
    with pytest.raises(_lib.MMCError, match="MMC_ERR_ARG"):
        _lib.check(st)


@pytest.mark.parametrize("kw,word", [
    (dict(r_hb=float("nan")), "r_hb"), (dict(r_hb=float("inf")), "r_hb"), (dict(r_hb=0.0), "r_hb"),
    (dict(r_hb=-3.5), "r_hb"),
    (dict(cos_hb=0.0), "cos_hb"), (dict(cos_hb=-0.5), "cos_hb"), (dict(cos_hb=math.nextafter(1.0, 2.0)), "cos_hb"),
    (dict(cos_hb=float("nan")), "cos_hb"),
    (dict(q_bins=0), "q_bins"), (dict(q_bins=-1), "q_bins"), (dict(q_bins=4097), "q_bins"),
    (dict(outputs=(False, False, False)), "at least one"),
])
def test_arguments_refused_without_a_device(kw, word):
    """These are refused before the batch is looked at: the message names the argument, not the
    NULL batch, and nothing is written."""
    st, msg = call(**kw)
    assert st == _lib.MMC_ERR_ARG
    assert word in msg and "batch is NULL" not in msg, msg
