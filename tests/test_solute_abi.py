"""CPU tests of the boundary of mmc_batch_widom_solute and mmc_batch_widom_solute_at: declared with
the agreed prototypes, exported, bound with matching ctypes, and loud on a NULL batch and on every
argument that can be refused without a device -- with the outputs coming back untouched."""
import ctypes as C
import re

import pytest

import boundary
from metropolismontecarlo_amd import _lib

PROTOTYPES = {
    "mmc_batch_widom_solute": (
        "int32_t mmc_batch_widom_solute(mmc_batch *b, int32_t n_sites, const double *offsets, const double *charge, "
        "const double *eps, const double *sig, int64_t n_insert, uint64_t seed, int64_t draw0, double temperature, "
        "double *boltz_sum, int64_t *n_overlap, double *mol_out, double *du_out, uint8_t *ovl_out);"),
    "mmc_batch_widom_solute_at": (
        "int32_t mmc_batch_widom_solute_at(mmc_batch *b, int32_t n_sites, const double *charge, const double *eps, "
        "const double *sig, int64_t n_insert, const double *mol_in, double temperature, double *boltz_sum, "
        "int64_t *n_overlap, double *du_out, uint8_t *ovl_out);"),
}


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_symbols_are_declared_exported_and_bound_with_the_header_prototype(name):
    """(Exported and bound with these types: tests/test_abi.py, for every function of the header.)"""
    assert boundary.prototype_text(name) == PROTOTYPES[name]


def test_the_constant_of_the_header_and_its_mirrors():
    import os
    from metropolismontecarlo_amd import structs
    assert re.search(r"#define\s+MMC_SOLUTE_MAX_SITES\s+16\b", boundary.header_code())
    assert structs.Solute.MAX_SITES == 16
    hpp = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "mmc_solute.hpp")).read()
    assert re.search(r"#define\s+SOL_MAX_SITES\s+16\b", hpp)


def call(at=False, b=None, S=2, n_sites=None, offsets=0.5, charge=(0.4, -0.4), eps=50.0, sig=3.0, n_insert=4,
         temperature=298.15, sums=(True, True), mol=1.0):
    """One call with sentinel outputs, which must come back untouched.  `offsets`, `eps`, `sig` and
    `mol`: a fill value, a sequence, or None for a NULL pointer.  Returns (status, message)."""
    def arr(v, n):
        if v is None:
            return None
        vals = list(v) if isinstance(v, (tuple, list)) else [v] * n
        return (C.c_double * max(len(vals), 1))(*vals)

    bs = (C.c_double * 4)(*([7.5] * 4))
    no = (C.c_int64 * 4)(*([3] * 4))
    du = (C.c_double * 64)(*([7.5] * 64))
    ov = (C.c_uint8 * 16)(*([9] * 16))
    mo = (C.c_double * 256)(*([7.5] * 256))
    n_sites = S if n_sites is None else n_sites
    q = arr(charge, S)
    L = _lib.lib()
    if at:
        st = L.mmc_batch_widom_solute_at(b, n_sites, q, arr(eps, 3 * S), arr(sig, 3 * S), n_insert,
                                         arr(mol, 3 * (S + 1) * 4), temperature, bs if sums[0] else None,
                                         no if sums[1] else None, du, ov)
    else:
        st = L.mmc_batch_widom_solute(b, n_sites, arr(offsets, 3 * S), q, arr(eps, 3 * S), arr(sig, 3 * S), n_insert,
                                      1234, 0, temperature, bs if sums[0] else None, no if sums[1] else None,
                                      mo, du, ov)
    assert all(v == 7.5 for v in bs) and all(v == 3 for v in no) and all(v == 7.5 for v in du)
    assert all(v == 9 for v in ov) and all(v == 7.5 for v in mo)
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
    (dict(n_sites=0), "n_sites"), (dict(n_sites=-1), "n_sites"), (dict(n_sites=17), "n_sites"),
    (dict(charge=None), "charge"), (dict(eps=None), "eps"), (dict(sig=None), "sig"),
    (dict(sums=(False, True)), "boltz_sum"), (dict(sums=(True, False)), "n_overlap"),
    (dict(n_insert=0), "n_insert"), (dict(n_insert=-2), "n_insert"),
    (dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"),
    (dict(temperature=NAN), "temperature"), (dict(temperature=INF), "temperature"),
    (dict(charge=(0.4, NAN)), "charge"), (dict(charge=(INF, 0.0)), "charge"),
    (dict(eps=NAN), "eps"), (dict(eps=INF), "eps"), (dict(eps=(1.0, 1.0, 1.0, 1.0, -1e-300, 1.0)), "eps"),
    (dict(sig=NAN), "sig"), (dict(sig=INF), "sig"), (dict(sig=(1.0, 1.0, 1.0, 1.0, 1.0, -3.0)), "sig"),
])
def test_arguments_refused_without_a_device(at, kw, word):
    """These are refused before the batch is looked at: the message names the argument, not the
    NULL batch, and nothing is written."""
    st, msg = call(at, **kw)
    assert st == _lib.MMC_ERR_ARG
    assert word in msg and "batch is NULL" not in msg, msg


@pytest.mark.parametrize("kw,word", [
    (dict(offsets=None), "offsets"), (dict(offsets=NAN), "offsets"),
    (dict(offsets=(0.0, 0.0, 0.0, 0.0, -INF, 0.0)), "offsets"),
])
def test_offsets_refused_without_a_device(kw, word):
    st, msg = call(False, **kw)
    assert st == _lib.MMC_ERR_ARG and word in msg and "batch is NULL" not in msg, msg


def test_null_molecules_are_refused_without_a_device():
    st, msg = call(True, mol=None)
    assert st == _lib.MMC_ERR_ARG and "mol_in" in msg and "batch is NULL" not in msg, msg


@pytest.mark.parametrize("at", [False, True])
def test_the_largest_solute_and_zero_parameters_get_as_far_as_the_batch(at):
    """16 sites, zero charges, eps = 0 and sig = 0 are all valid: the call reaches the batch."""
    st, msg = call(at, S=16, charge=0.0, eps=0.0, sig=0.0, mol=2.0, n_insert=1)
    assert st == _lib.MMC_ERR_ARG and "batch is NULL" in msg, msg
