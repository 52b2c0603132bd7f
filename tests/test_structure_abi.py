"""CPU tests of the boundary of mmc_batch_rdf_sites and mmc_batch_dipoles: loud on a NULL batch and on
every argument that can be refused without a device, as every later observable is
(tests/test_orient_abi.py), and called by the Julia binding."""
import ctypes as C

import pytest

import boundary
from metropolismontecarlo_amd import _lib

NAMES = ("mmc_batch_rdf_sites", "mmc_batch_dipoles")
MAX_BINS = 2046          # include/mmc_hip.h, "Structure observables": what one wave's histograms may take
SENTINEL = 0x0123456789abcdef
SENTINEL_F = -1234.5


def last_error():
    msg = _lib.lib().mmc_last_error()
    return msg.decode() if msg else ""


def rdf_sites(b=None, numbins=10, r_max=0.0, per_replica=0, hist=True):
    h = (C.c_uint64 * 96)(*([SENTINEL] * 96))
    st = _lib.lib().mmc_batch_rdf_sites(b, numbins, r_max, per_replica, h if hist else None)
    assert all(v == SENTINEL for v in h)
    return st, last_error()


def dipoles(b=None, dip=True):
    d = (C.c_double * 12)(*([SENTINEL_F] * 12))
    st = _lib.lib().mmc_batch_dipoles(b, d if dip else None)
    assert all(v == SENTINEL_F for v in d)
    return st, last_error()


def test_the_julia_binding_calls_them():
    assert set(NAMES) <= boundary.julia_bound()


def test_a_null_batch_fails_loudly():
    for st, msg in (rdf_sites(), rdf_sites(numbins=MAX_BINS, r_max=3.0, per_replica=1), dipoles()):
        assert st == _lib.MMC_ERR_ARG and "batch is NULL" in msg
        with pytest.raises(_lib.MMCError, match="MMC_ERR_ARG"):
            _lib.check(st)


@pytest.mark.parametrize("fn,kw,word", [
    (rdf_sites, dict(hist=False), "NULL out pointer"),
    (rdf_sites, dict(numbins=0), "numbins"), (rdf_sites, dict(numbins=-7), "numbins"),
    (rdf_sites, dict(numbins=MAX_BINS + 1), "numbins"), (rdf_sites, dict(numbins=2 ** 31 - 1), "numbins"),
    (rdf_sites, dict(r_max=float("nan")), "r_max"), (rdf_sites, dict(r_max=float("inf")), "r_max"),
    (rdf_sites, dict(r_max=-float("inf")), "r_max"),
    (dipoles, dict(dip=False), "NULL out pointer"),
])
def test_arguments_refused_without_a_device(fn, kw, word):
    """These are refused before the batch is looked at: the message names the call and the argument, not
    the NULL batch, and nothing is written.  (An r_max against the boxes needs the batch:
    tests/test_gpu_structure.py.)"""
    st, msg = fn(**kw)
    assert st == _lib.MMC_ERR_ARG
    assert word in msg and "batch is NULL" not in msg, msg
    assert msg.startswith("mmc_batch_rdf_sites" if fn is rdf_sites else "mmc_batch_dipoles"), msg
