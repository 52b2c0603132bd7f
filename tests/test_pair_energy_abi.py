"""CPU tests of mmc_batch_pair_energy's boundary: declared with the agreed prototype, exported, bound
with matching ctypes, called by the Julia binding, loud on a NULL batch and on every argument that can
be refused without a device, and the Python wrapper's own check of `out`."""
import ctypes as C

import numpy as np
import pytest

import boundary
from boundary import header_define
from common import fake_batch
from metropolismontecarlo_amd import _lib

NAME = "mmc_batch_pair_energy"
PROTOTYPE = ("int32_t mmc_batch_pair_energy(mmc_batch *b, int32_t numbins, double r_max, int32_t n_ebins, "
             "double u_lo, double u_hi, double u_hb, int32_t per_replica, int64_t *rows, uint64_t *uhist, "
             "uint64_t *nhb, uint64_t *flagged);")
SENTINEL = 0x0123456789abcdef


def test_symbol_is_declared_exported_and_bound_with_the_header_prototype():
    """(Exported and bound with these types: tests/test_abi.py, for every function of the header.)"""
    assert boundary.prototype_text(NAME) == PROTOTYPE


def test_the_header_states_the_definition_and_its_constants():
    src = boundary.header_text()
    sec = src[src.index("Pair-energy distributions"):src.index("int32_t mmc_batch_pair_energy")]
    assert src.index("Orientational pair correlations") < src.index("Pair-energy distributions") \
        < src.index("Partial structure factors")
    for cite in ("exactly mmc_batch_orient_corr's", "gr.jl:75-80", "e_a(m) = vector1D(site 0 of m, atom a of m)",
                 "x_ab = (D + e_a(i)) - e_b(j)", "r2_ab = (x x + y y) + z z", "(q_a * q_b) / sqrt(r2_ab)",
                 "(4.0 * eps_ab) * (s6 * s6 - s6)", "s6 = (s2 * s2) * s2", "s2 = (sig_ab * sig_ab) / r2_ab",
                 "eps_ab > 0.001", "u    = u_C + u_LJ", "2^-21 K", "magnitude >= 2^20 K", "ties to even",
                 "rows 1 and 2 of slot numbins + 1 are 0", "mmc_batch_deletion's rule", "MMC_PAIRE_NHB - 1 = 8",
                 "rows[R][3][numbins + 2]", "MMC_ERR_STATE", "MMC_ERR_UNSUPPORTED", "MMC_PAIRE_MAX_BINS",
                 "tests/pair_energy_ref.py"):
        assert cite in sec, cite
    assert float(header_define("MMC_PAIRE_SCALE")) == 2.0 ** 20
    assert int(header_define("MMC_PAIRE_NHB")) == 9
    max_e = int(header_define("MMC_PAIRE_MAX_EBINS"))
    assert max_e == 4096
    # what one wave fits in 64 KB, all 64-bit: thresholds and three rows per slot, the LJ constants of nine
    # atom pairs (144 bytes), the largest energy histogram and the flagged count
    max_bins = int(header_define("MMC_PAIRE_MAX_BINS"))
    fixed = 144 + 8 * (max_e + 2) + 8
    assert 32 * (max_bins + 2) + fixed <= 65536 < 32 * (max_bins + 3) + fixed


def test_the_julia_binding_calls_it():
    assert NAME in boundary.julia_bound()


def call(b=None, numbins=10, r_max=0.0, n_ebins=8, u_lo=-4000.0, u_hi=2000.0, u_hb=-1132.2, per_replica=0,
         rows=True, uhist=True, nhb=True, flagged=True):
    bufs = [(C.c_int64 * 64)(*([SENTINEL] * 64))] + [(C.c_uint64 * 64)(*([SENTINEL] * 64)) for _ in range(3)]
    args = [buf if given else None for buf, given in zip(bufs, (rows, uhist, nhb, flagged))]
    st = _lib.lib().mmc_batch_pair_energy(b, numbins, r_max, n_ebins, u_lo, u_hi, u_hb, per_replica, *args)
    assert all(v == SENTINEL for buf in bufs for v in buf)
    msg = _lib.lib().mmc_last_error()
    return st, (msg.decode() if msg else "")


def test_a_null_batch_fails_loudly():
    st, msg = call()
    assert st == _lib.MMC_ERR_ARG and "batch is NULL" in msg
    with pytest.raises(_lib.MMCError, match="MMC_ERR_ARG"):
        _lib.check(st)
    st, msg = call(numbins=int(header_define("MMC_PAIRE_MAX_BINS")), r_max=3.0, n_ebins=4096, per_replica=1)
    assert st == _lib.MMC_ERR_ARG and "batch is NULL" in msg
    # what is ignored without its output is not looked at
    st, msg = call(uhist=False, n_ebins=0, u_lo=float("nan"), u_hi=float("nan"))
    assert st == _lib.MMC_ERR_ARG and "batch is NULL" in msg
    st, msg = call(nhb=False, u_hb=float("nan"))
    assert st == _lib.MMC_ERR_ARG and "batch is NULL" in msg


@pytest.mark.parametrize("kw,word", [
    (dict(rows=False), "rows"), (dict(flagged=False), "flagged"),
    (dict(numbins=0), "numbins"), (dict(numbins=-7), "numbins"),
    (dict(numbins=1017), "numbins"), (dict(numbins=2 ** 31 - 1), "numbins"),
    (dict(r_max=float("nan")), "r_max"), (dict(r_max=float("inf")), "r_max"), (dict(r_max=-float("inf")), "r_max"),
    (dict(n_ebins=0), "n_ebins"), (dict(n_ebins=-1), "n_ebins"), (dict(n_ebins=4097), "n_ebins"),
    (dict(u_lo=2000.0, u_hi=2000.0), "u_lo"), (dict(u_lo=1.0, u_hi=-1.0), "u_lo"),
    (dict(u_lo=float("nan")), "u_lo"), (dict(u_hi=float("inf")), "u_hi"), (dict(u_lo=-float("inf")), "u_lo"),
    (dict(u_hb=float("nan")), "u_hb"), (dict(u_hb=float("inf")), "u_hb"), (dict(u_hb=-float("inf")), "u_hb"),
])
def test_arguments_refused_without_a_device(kw, word):
    """These are refused before the batch is looked at: the message names the argument, not the NULL
    batch, and nothing is written.  (An r_max against the boxes needs the batch:
    tests/test_gpu_pair_energy.py.)"""
    assert int(header_define("MMC_PAIRE_MAX_BINS")) == 1016
    st, msg = call(**kw)
    assert st == _lib.MMC_ERR_ARG
    assert word in msg and "batch is NULL" not in msg, msg


# (device.Batch.pair_energy's own check of `out` runs before the library is called.)
def _out(**kw):
    good = dict(rows=np.zeros((3, 12), dtype=np.int64), uhist=np.zeros(8, dtype=np.uint64),
                nhb=np.zeros(9, dtype=np.uint64), flagged=np.zeros(1, dtype=np.uint64))
    good.update(kw)
    return good


@pytest.mark.parametrize("kw", [
    dict(out=_out(rows=np.zeros((3, 12), dtype=np.uint64))), dict(out=_out(rows=np.zeros((3, 11), dtype=np.int64))),
    dict(out=_out(rows=np.zeros((2, 3, 12), dtype=np.int64))),
    dict(out=_out(rows=np.zeros((3, 24), dtype=np.int64)[:, ::2])), dict(out=_out(rows=[[0] * 12] * 3)),
    dict(out=_out(uhist=np.zeros(7, dtype=np.uint64))), dict(out=_out(uhist=np.zeros(8, dtype=np.int64))),
    dict(out=_out(nhb=np.zeros(8, dtype=np.uint64))), dict(out=_out(flagged=np.zeros(2, dtype=np.uint64))),
    dict(out=_out(flagged=np.zeros(1, dtype=np.int64))), dict(out=_out(), per_replica=True),
    dict(out=_out(extra=np.zeros(1))), dict(out=np.zeros((3, 12), dtype=np.int64)),
])
def test_the_wrapper_checks_its_arguments(kw):
    with pytest.raises(ValueError):
        fake_batch("pair_energy").pair_energy(10, n_ebins=6, u_hb=-1132.2, **kw)
    with pytest.raises(AssertionError, match="the library was reached"):
        fake_batch("pair_energy").pair_energy(10, n_ebins=6, u_hb=-1132.2, out=_out())


def test_the_wrapper_refuses_outputs_that_were_not_asked_for():
    with pytest.raises(ValueError):
        fake_batch("pair_energy").pair_energy(10, out=_out())                 # no energy bins, no u_hb: uhist and nhb are not outputs
    with pytest.raises(AssertionError, match="the library was reached"):
        fake_batch("pair_energy").pair_energy(10, out=dict(rows=np.zeros((3, 12), dtype=np.int64)))
