"""CPU tests of mmc_batch_shell_order's boundary: declared with the agreed prototype, exported,
bound with matching ctypes, and loud on a NULL batch and on every argument that can be refused
without a device."""
import ctypes as C
import math

import pytest

import boundary
from metropolismontecarlo_amd import _lib

NAME = "mmc_batch_shell_order"
PROTOTYPE = ("int32_t mmc_batch_shell_order(mmc_batch *b, double r_list, double r_lsi, double r_ang, double r_hb, "
             "double cos_hb, int32_t n_rank, int32_t r_bins, int32_t lsi_bins, double lsi_max, int32_t ang_bins, "
             "int32_t zeta_bins, double zeta_lo, double zeta_hi, int32_t per_replica, "
             "uint64_t *rank_hist, uint64_t *lsi_hist, uint64_t *ang_hist, uint64_t *zeta_hist, uint64_t *flagged, "
             "double *sums, int32_t *count_out, int32_t *nbr_out, double *lsi_out, double *zeta_out);")
INF, NAN = float("inf"), float("nan")


def test_symbol_is_declared_exported_and_bound_with_the_header_prototype():
    """(Exported and bound with these types: tests/test_abi.py, for every function of the header.)"""
    assert boundary.prototype_text(NAME) == PROTOTYPE
    assert len(boundary.header_prototypes()[NAME][1]) == 25


def test_the_julia_binding_and_the_python_method_carry_it():
    import inspect
    from metropolismontecarlo_amd.device import Batch
    jl = boundary.julia_text()
    assert ":mmc_batch_shell_order" in jl and "function shell_order(" in jl
    sig = inspect.signature(Batch.shell_order)
    assert [(k, p.default) for k, p in sig.parameters.items()][1:] == [
        ("r_list", 6.0), ("r_lsi", 3.7), ("r_ang", 3.3), ("r_hb", 3.5), ("theta_deg", 30.0), ("n_rank", 8),
        ("r_bins", 300), ("lsi_bins", 200), ("lsi_max", 0.4), ("ang_bins", 180), ("zeta_bins", 200),
        ("zeta_lo", -1.5), ("zeta_hi", 2.5), ("per_replica", False), ("details", False), ("out", None)]


SIZE = 16 * 1025


def call(b=None, r_list=6.0, r_lsi=3.7, r_ang=3.3, r_hb=3.5, cos_hb=math.cos(math.radians(30.0)), n_rank=8, r_bins=300,
         lsi_bins=200, lsi_max=0.4, ang_bins=180, zeta_bins=200, zeta_lo=-1.5, zeta_hi=2.5,
         outputs=(True, True, True, True, True)):
    hists = [(C.c_uint64 * SIZE)(*([77] * SIZE)) for _ in range(4)]
    fl = (C.c_uint64 * 2)(77, 77)
    sums = (C.c_double * 8)(*([7.5] * 8))
    st = _lib.lib().mmc_batch_shell_order(
        b, r_list, r_lsi, r_ang, r_hb, cos_hb, n_rank, r_bins, lsi_bins, lsi_max, ang_bins, zeta_bins, zeta_lo, zeta_hi,
        0, *[h if on else None for h, on in zip(hists, outputs)], fl, sums if outputs[4] else None,
        None, None, None, None)
    assert all(v == 77 for h in hists for v in h) and list(fl) == [77, 77] and list(sums) == [7.5] * 8
    msg = _lib.lib().mmc_last_error()
    return st, (msg.decode() if msg else "")


def test_a_null_batch_fails_loudly():
    st, msg = call()
    assert st == _lib.MMC_ERR_ARG and "NULL" in msg
    with pytest.raises(_lib.MMCError, match="MMC_ERR_ARG"):
        _lib.check(st)
    # the largest bins that fit a wave's counters pass the argument checks too
    st, msg = call(n_rank=1, r_bins=1024, lsi_bins=1024, ang_bins=1024, zeta_bins=1024)
    assert st == _lib.MMC_ERR_ARG and "NULL" in msg
    st, msg = call(n_rank=16, r_bins=1024, outputs=(False, True, True, True, True))    # rank_hist NULL: no counters
    assert st == _lib.MMC_ERR_ARG and "NULL" in msg
    st, msg = call(n_rank=7, r_bins=1023, lsi_bins=276, ang_bins=276, zeta_bins=276)   # 7999 bins: the bound itself
    assert st == _lib.MMC_ERR_ARG and "NULL" in msg


@pytest.mark.parametrize("kw,word", [
    (dict(r_list=NAN), "r_list"), (dict(r_list=INF), "r_list"), (dict(r_list=0.0), "r_list"), (dict(r_list=-6.0), "r_list"),
    (dict(r_lsi=0.0), "r_lsi"), (dict(r_lsi=NAN), "r_lsi"), (dict(r_lsi=math.nextafter(6.0, 7.0)), "r_lsi"),
    (dict(r_ang=0.0), "r_ang"), (dict(r_ang=NAN), "r_ang"), (dict(r_ang=6.5), "r_ang"), (dict(r_ang=-1.0), "r_ang"),
    (dict(r_hb=0.0), "r_hb"), (dict(r_hb=NAN), "r_hb"), (dict(r_hb=INF), "r_hb"),
    (dict(cos_hb=0.0), "cos_hb"), (dict(cos_hb=-0.5), "cos_hb"), (dict(cos_hb=math.nextafter(1.0, 2.0)), "cos_hb"),
    (dict(cos_hb=NAN), "cos_hb"),
    (dict(n_rank=0), "n_rank"), (dict(n_rank=17), "n_rank"), (dict(n_rank=-1), "n_rank"),
    (dict(r_bins=0), "r_bins"), (dict(r_bins=1025), "r_bins"),
    (dict(lsi_bins=0), "lsi_bins"), (dict(lsi_bins=1025), "lsi_bins"),
    (dict(lsi_max=0.0), "lsi_max"), (dict(lsi_max=-0.4), "lsi_max"), (dict(lsi_max=NAN), "lsi_max"),
    (dict(lsi_max=INF), "lsi_max"),
    (dict(ang_bins=0), "ang_bins"), (dict(ang_bins=1025), "ang_bins"),
    (dict(zeta_bins=0), "zeta_bins"), (dict(zeta_bins=-7), "zeta_bins"), (dict(zeta_bins=1025), "zeta_bins"),
    (dict(zeta_lo=2.5), "zeta_lo"), (dict(zeta_lo=3.0), "zeta_lo"), (dict(zeta_lo=NAN), "zeta_lo"),
    (dict(zeta_hi=INF), "zeta_hi"), (dict(zeta_lo=-INF), "zeta_lo"),
    (dict(outputs=(False, False, False, False, False)), "at least one"),
    (dict(n_rank=16, r_bins=1024), "bins"),                                            # 16400 counters of the ranks alone
    (dict(n_rank=7, r_bins=1023, lsi_bins=277, ang_bins=276, zeta_bins=276), "bins"),  # 8000: one too many
])
def test_arguments_refused_without_a_device(kw, word):
    """These are refused before the batch is looked at: the message names the argument, not the
    NULL batch, and nothing is written."""
    st, msg = call(**kw)
    assert st == _lib.MMC_ERR_ARG
    assert word in msg and "batch is NULL" not in msg, msg
