"""CPU tests of mmc_batch_volume_perturb's boundary: declared with the agreed prototype, exported,
bound with matching ctypes, and loud on a NULL batch and on every argument that can be refused
without a device."""
import ctypes as C

import pytest

import boundary
from metropolismontecarlo_amd import _lib

NAME = "mmc_batch_volume_perturb"
PROTOTYPE = ("int32_t mmc_batch_volume_perturb(mmc_batch *b, int32_t n_scale, const double *scale, "
             "double temperature, double *boltz_sum, int64_t *n_overlap, double *du_out, "
             "double *base_out);")


def test_symbol_is_declared_exported_and_bound_with_the_header_prototype():
    """(Exported and bound with these types: tests/test_abi.py, for every function of the header.)"""
    assert boundary.prototype_text(NAME) == PROTOTYPE


def test_the_header_states_the_definition_with_its_reference_lines():
    src = boundary.header_text()
    sec = src[src.index("Virtual volume moves"):src.index("int32_t mmc_batch_volume_perturb")]
    for cite in ("volumeChange.jl:62-80", "volumeChange.jl:129-130", "main.jl:290-291",
                 "Ewald/energy.jl:946-1032", "Ewald/ewalds.jl:45-103", "Ewald/ewalds.jl:829-833",
                 "ewalds.jl:359", "Order of summation"):
        assert cite in sec, cite


def call(b=None, scale=(0.99, 1.01), n_scale=None, temperature=298.15, outputs=(True, True, True, True)):
    K = 8
    sc = None if scale is None else (C.c_double * K)(*(list(scale) + [1.0] * (K - len(scale))))
    bs = (C.c_double * (2 * K))(*([7.5] * (2 * K)))
    no = (C.c_int64 * (2 * K))(*([77] * (2 * K)))
    du = (C.c_double * (8 * K))(*([7.5] * (8 * K)))
    base = (C.c_double * 8)(*([7.5] * 8))
    n = len(scale) if n_scale is None else n_scale
    st = _lib.lib().mmc_batch_volume_perturb(b, n, sc, temperature, bs if outputs[0] else None,
                                             no if outputs[1] else None, du if outputs[2] else None,
                                             base if outputs[3] else None)
    assert all(v == 7.5 for v in bs) and all(v == 77 for v in no)
    assert all(v == 7.5 for v in du) and all(v == 7.5 for v in base)
    msg = _lib.lib().mmc_last_error()
    return st, (msg.decode() if msg else "")


def test_a_null_batch_fails_loudly():
    st, msg = call()
    assert st == _lib.MMC_ERR_ARG and "NULL" in msg
    with pytest.raises(_lib.MMCError, match="MMC_ERR_ARG"):
        _lib.check(st)


@pytest.mark.parametrize("kw,word", [
    (dict(n_scale=0), "n_scale"), (dict(n_scale=-1), "n_scale"), (dict(n_scale=9), "n_scale"),
    (dict(scale=None, n_scale=2), "scale is NULL"),
    (dict(scale=(0.99, float("nan"))), "scale[1]"), (dict(scale=(float("inf"),)), "scale[0]"),
    (dict(scale=(1.0, 1.01, 0.0)), "scale[2]"), (dict(scale=(-0.99,)), "scale[0]"),
    (dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"),
    (dict(temperature=float("nan")), "temperature"), (dict(temperature=float("inf")), "temperature"),
    (dict(outputs=(False, False, False, False)), "at least one"),
])
def test_arguments_refused_without_a_device(kw, word):
    """These are refused before the batch is looked at: the message names the argument, not the
    NULL batch, and nothing is written.  (L_k < 2 r_cut needs the batch's box: tests/
    test_gpu_volume_perturb.py.)"""
    st, msg = call(**kw)
    assert st == _lib.MMC_ERR_ARG
    assert word in msg and "batch is NULL" not in msg, msg
