"""CPU tests of mmc_batch_bond_order's boundary: declared with the agreed prototype, exported, bound
with matching ctypes, carried by the Julia binding and the Python method, and loud on a NULL batch and
on every argument that can be refused without a device."""
import ctypes as C
import re

import pytest

import boundary
from metropolismontecarlo_amd import _lib

NAME = "mmc_batch_bond_order"
PROTOTYPE = ("int32_t mmc_batch_bond_order(mmc_batch *b, int32_t l, double r_nb, int32_t n_nb, double a_lo, double a_hi, "
             "double b_lo, double b_hi, int32_t min_a, int32_t min_ab, int32_t q_bins, int32_t c_bins, "
             "int32_t per_replica, uint64_t *q_hist, uint64_t *qbar_hist, uint64_t *c_hist, uint64_t *ab_hist, "
             "uint64_t *size_hist, int64_t *stats, double *sums, double *q_out, double *qbar_out, "
             "int32_t *nbr_out, uint8_t *ab_out, int32_t *label_out);")
INF, NAN = float("inf"), float("nan")


def test_symbol_is_declared_exported_and_bound_with_the_header_prototype():
    """(Exported and bound with these types: tests/test_abi.py, for every function of the header.)"""
    assert boundary.prototype_text(NAME) == PROTOTYPE
    assert len(boundary.header_prototypes()[NAME][1]) == 25


def test_the_header_fixes_the_limits_and_the_definitions():
    text = boundary.header_text()
    for macro, value in (("MMC_BO_MAX_NB", 16), ("MMC_BO_MAX_BINS", 4096), ("MMC_BO_STATS", 8), ("MMC_BO_MAX_MOL", 8000)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), text), macro
    sec = text[text.index("---- Bond order"):text.index("int32_t mmc_batch_bond_order")]
    for word in ("T_n^m", "c_m = x c_(m-1) - y s_(m-1)", "PI = 3.141592653589793", "rank order", "bond_chunk"):
        assert word in sec, word
    assert not re.search(r"\b(sin|cos|acos|atan2?)\s*\(", sec)      # no trigonometry in the definitions


def test_the_julia_binding_and_the_python_method_carry_it():
    import inspect
    from metropolismontecarlo_amd import observables as obs
    from metropolismontecarlo_amd.device import Batch
    jl = boundary.julia_text()
    assert ":mmc_batch_bond_order" in jl and "function bond_order(" in jl
    sig = inspect.signature(Batch.bond_order)
    assert [(k, p.default) for k, p in sig.parameters.items()][1:] == [
        ("l", 3), ("r_nb", 3.5), ("n_nb", 4), ("a", (-INF, -0.8)), ("b", (-0.35, 0.25)), ("min_a", 3), ("min_ab", 4),
        ("q_bins", 200), ("c_bins", 200), ("per_replica", False), ("details", False), ("out", None)]
    for fn in ("steinhardt_distribution", "bond_correlation_distribution", "solid_fraction", "largest_nucleus",
               "nucleus_size_distribution", "chill_plus_classes"):
        assert callable(getattr(obs, fn)), fn
    doc = obs.chill_plus_classes.__doc__
    assert all(w in doc for w in ("S = 4", "S = 3 and E = 1", "E = 4", "E = 3", "S = 2", "Nguyen and Molinero"))


SIZE = 4097
OUTPUTS = ("q_hist", "qbar_hist", "c_hist", "ab_hist", "size_hist", "stats", "sums", "q", "qbar", "nbr", "ab", "label")


def call(b=None, l=3, r_nb=3.5, n_nb=4, a_lo=-INF, a_hi=-0.8, b_lo=-0.35, b_hi=0.25, min_a=3, min_ab=4, q_bins=200,
         c_bins=200, outputs=OUTPUTS[:7]):
    hists = [(C.c_uint64 * SIZE)(*([77] * SIZE)) for _ in range(5)]
    stats = (C.c_int64 * 16)(*([-7] * 16))
    dbl = [(C.c_double * 8)(*([7.5] * 8)) for _ in range(3)]
    nbr, lab = (C.c_int32 * 32)(*([-5] * 32)), (C.c_int32 * 2)(-5, -5)
    ab = (C.c_uint8 * 4)(9, 9, 9, 9)
    every = dict(zip(OUTPUTS, hists + [stats] + dbl + [nbr, ab, lab]))
    st = _lib.lib().mmc_batch_bond_order(b, l, r_nb, n_nb, a_lo, a_hi, b_lo, b_hi, min_a, min_ab, q_bins, c_bins, 0,
                                         *[every[k] if k in outputs else None for k in OUTPUTS])
    assert all(v == 77 for h in hists for v in h) and all(v == -7 for v in stats)
    assert all(v == 7.5 for d in dbl for v in d) and all(v == -5 for v in nbr) and list(lab) == [-5, -5]
    assert list(ab) == [9] * 4
    msg = _lib.lib().mmc_last_error()
    return st, (msg.decode() if msg else "")


def test_a_null_batch_fails_loudly():
    st, msg = call()
    assert st == _lib.MMC_ERR_ARG and "NULL" in msg
    with pytest.raises(_lib.MMCError, match="MMC_ERR_ARG"):
        _lib.check(st)
    # the limits themselves, infinite window bounds and one output of any kind pass the argument checks
    for kw in (dict(l=6, n_nb=16, q_bins=4096, c_bins=4096), dict(l=4, n_nb=1, q_bins=1, c_bins=1),
               dict(a_lo=-INF, a_hi=INF, b_lo=-INF, b_hi=INF), dict(min_a=0, min_ab=0), dict(min_a=-1, min_ab=99)):
        st, msg = call(**kw)
        assert st == _lib.MMC_ERR_ARG and "batch is NULL" in msg, (kw, msg)
    for k in OUTPUTS:
        st, msg = call(outputs=(k,))
        assert st == _lib.MMC_ERR_ARG and "batch is NULL" in msg, (k, msg)


@pytest.mark.parametrize("kw,word", [
    (dict(l=0), "l must"), (dict(l=2), "l must"), (dict(l=5), "l must"), (dict(l=7), "l must"), (dict(l=-3), "l must"),
    (dict(r_nb=NAN), "r_nb"), (dict(r_nb=INF), "r_nb"), (dict(r_nb=0.0), "r_nb"), (dict(r_nb=-3.5), "r_nb"),
    (dict(n_nb=0), "n_nb"), (dict(n_nb=17), "n_nb"), (dict(n_nb=-4), "n_nb"),
    (dict(q_bins=-1), "q_bins"), (dict(q_bins=0), "q_bins"), (dict(q_bins=4097), "q_bins"),
    (dict(c_bins=-1), "c_bins"), (dict(c_bins=0), "c_bins"), (dict(c_bins=4097), "c_bins"),
    (dict(a_lo=NAN), "a_lo"), (dict(a_hi=NAN), "a_hi"), (dict(b_lo=NAN), "b_lo"), (dict(b_hi=NAN), "b_hi"),
    (dict(outputs=()), "at least one"),
])
def test_arguments_refused_without_a_device(kw, word):
    """These are refused before the batch is looked at: the message names the argument, not the
    NULL batch, and nothing is written."""
    st, msg = call(**kw)
    assert st == _lib.MMC_ERR_ARG
    assert word in msg and "batch is NULL" not in msg, msg
