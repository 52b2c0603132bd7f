"""CPU tests of mmc_batch_deletion's boundary: declared with the agreed prototype, exported, bound
with matching ctypes, loud on a NULL batch and on every argument that can be refused without a
device, and the Python wrapper's own argument checks."""
import ctypes as C

import numpy as np
import pytest

import boundary
from common import fake_batch
from metropolismontecarlo_amd import _lib

NAME = "mmc_batch_deletion"
PROTOTYPE = ("int32_t mmc_batch_deletion(mmc_batch *b, int32_t n_sel, const int32_t *sel, double temperature, "
             "int32_t n_bins, double u_lo, double u_hi, int32_t per_replica, uint64_t *hist, double *esum, "
             "double *boltz_sum, int64_t *n_flagged, double *du_out, uint8_t *ovl_out);")


def test_symbol_is_declared_exported_and_bound_with_the_header_prototype():
    """(Exported and bound with these types: tests/test_abi.py, for every function of the header.)"""
    assert boundary.prototype_text(NAME) == PROTOTYPE


def test_the_header_states_the_definition_with_its_reference_lines():
    src = boundary.header_text()
    sec = src[src.index("Deletion energies"):src.index("int32_t mmc_batch_deletion")]
    for cite in ("Ewald/energy.jl:946-1032", "energy.jl:209-290", "ewalds.jl:892-910", ":293-376", ":359-360",
                 ":538-604", ":829-833", "mmc_batch_widom_at", "observables.ewald_intra_energy",
                 "2 Re(conj(S_k) s_k) - |s_k|^2", "esum[r][0] == 2 lj", "floor((dU - u_lo) * s)"):
        assert cite in sec, cite


def test_the_julia_binding_calls_it():
    assert NAME in boundary.julia_bound()


def call(b=None, sel=None, n_sel=0, temperature=298.15, bins=(10, -1.0, 1.0), outputs=(True,) * 6):
    hist = (C.c_uint64 * 4100)(*([77] * 4100))
    esum = (C.c_double * 8)(*([7.5] * 8))
    bs = (C.c_double * 2)(7.5, 7.5)
    nf = (C.c_int64 * 2)(77, 77)
    du = (C.c_double * 24)(*([7.5] * 24))
    ovl = (C.c_uint8 * 8)(*([9] * 8))
    sel_a = None if sel is None else (C.c_int32 * max(len(sel), 1))(*sel)
    outs = [x if on else None for x, on in zip((hist, esum, bs, nf, du, ovl), outputs)]
    st = _lib.lib().mmc_batch_deletion(b, n_sel, sel_a, temperature, bins[0], bins[1], bins[2], 0, *outs)
    assert all(v == 77 for v in hist) and all(v == 7.5 for v in esum) and all(v == 7.5 for v in bs)
    assert all(v == 77 for v in nf) and all(v == 7.5 for v in du) and all(v == 9 for v in ovl)
    msg = _lib.lib().mmc_last_error()
    return st, (msg.decode() if msg else "")


def test_a_null_batch_fails_loudly():
    st, msg = call()
    assert st == _lib.MMC_ERR_ARG and "NULL" in msg
    with pytest.raises(_lib.MMCError, match="MMC_ERR_ARG"):
        _lib.check(st)


@pytest.mark.parametrize("kw,word", [
    (dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"),
    (dict(temperature=float("nan")), "temperature"), (dict(temperature=float("inf")), "temperature"),
    (dict(outputs=(False,) * 6), "every output is NULL"),
    (dict(bins=(0, -1.0, 1.0)), "n_bins"), (dict(bins=(-3, -1.0, 1.0)), "n_bins"),
    (dict(bins=(4097, -1.0, 1.0)), "n_bins"),
    (dict(bins=(10, 1.0, 1.0)), "u_lo < u_hi"), (dict(bins=(10, 2.0, 1.0)), "u_lo < u_hi"),
    (dict(bins=(10, float("nan"), 1.0)), "u_lo < u_hi"), (dict(bins=(10, -1.0, float("inf"))), "u_lo < u_hi"),
    (dict(bins=(10, float("-inf"), 1.0)), "u_lo < u_hi"),
    (dict(sel=[], n_sel=0), "n_sel"), (dict(sel=[3], n_sel=-2), "n_sel"),
])
def test_arguments_refused_without_a_device(kw, word):
    """These are refused before the batch is looked at: the message names the argument, not the
    NULL batch, and nothing is written.  (An index outside 0..N-1 needs the batch: tests/
    test_gpu_deletion.py.)"""
    st, msg = call(**kw)
    assert st == _lib.MMC_ERR_ARG
    assert word in msg and "batch is NULL" not in msg, msg


def test_a_grid_is_not_looked_at_without_a_histogram():
    """hist == NULL: n_bins and the bounds are ignored, the call gets as far as the NULL batch."""
    st, msg = call(bins=(0, float("nan"), 0.0), outputs=(False, True, True, True, True, True))
    assert st == _lib.MMC_ERR_ARG and "batch is NULL" in msg


# (device.Batch.deletion's own argument checks run before the library is called.)
@pytest.mark.parametrize("kw", [
    dict(sel=np.zeros((2, 2), dtype=np.int64)), dict(sel=np.array([0.5, 1.0])), dict(sel=np.array([2 ** 40])),
    dict(boltz_sum=np.zeros(3)), dict(boltz_sum=np.zeros(2, dtype=np.float32)), dict(boltz_sum=[0.0, 0.0]),
    dict(n_flagged=np.zeros(2)), dict(n_flagged=np.zeros(4, dtype=np.int64)[::2]),
])
def test_the_wrapper_checks_its_arguments(kw):
    with pytest.raises(ValueError):
        fake_batch("deletion").deletion(298.15, **kw)
