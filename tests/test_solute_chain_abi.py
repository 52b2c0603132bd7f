"""CPU tests of the boundary of the fixed-solute entry points (include/mmc_hip.h, "A fixed solute"):
declared with the agreed prototypes, exported, bound with matching ctypes, and loud on a NULL batch
and on every argument that can be refused without a device, in the documented order."""
import ctypes as C

import pytest

import boundary
from metropolismontecarlo_amd import _lib

PROTOTYPES = {
    "mmc_batch_set_solute": (
        "int32_t mmc_batch_set_solute(mmc_batch *b, int32_t n_sites, const double *mol, const double *charge, "
        "const double *eps, const double *sig);"),
    "mmc_batch_get_solute": (
        "int32_t mmc_batch_get_solute(mmc_batch *b, int32_t *n_sites, double *mol, double *charge, double *eps, "
        "double *sig);"),
    "mmc_batch_solute_energy": (
        "int32_t mmc_batch_solute_energy(mmc_batch *b, double *u_lj, double *u_real, uint8_t *ovl);"),
    "mmc_batch_rdf_solute": (
        "int32_t mmc_batch_rdf_solute(mmc_batch *b, int32_t numbins, double r_max, int32_t per_replica, "
        "uint64_t *hist);"),
}


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_symbols_are_declared_exported_and_bound_with_the_header_prototype(name):
    """(Exported and bound with these types: tests/test_abi.py, for every function of the header.)"""
    assert boundary.prototype_text(name) == PROTOTYPES[name]


def test_the_binding_and_the_julia_module_name_every_entry():
    from metropolismontecarlo_amd import device
    for method in ("set_solute", "get_solute", "solute_energy", "rdf_solute"):
        assert callable(getattr(device.Batch, method))
    bound = boundary.julia_bound()
    for name in PROTOTYPES:
        assert name in bound, name


def set_solute(b=None, S=2, n_sites=None, mol=1.0, charge=(0.4, -0.4), eps=50.0, sig=3.0):
    """One mmc_batch_set_solute; `mol`, `eps`, `sig`: a fill value, a sequence, or None for a NULL
    pointer.  Returns (status, message)."""
    def arr(v, n):
        if v is None:
            return None
        vals = list(v) if isinstance(v, (tuple, list)) else [v] * n
        return (C.c_double * max(len(vals), 1))(*vals)

    L = _lib.lib()
    st = L.mmc_batch_set_solute(b, S if n_sites is None else n_sites, arr(mol, 3 * (S + 1)), arr(charge, S),
                                arr(eps, 3 * S), arr(sig, 3 * S))
    msg = L.mmc_last_error()
    return st, (msg.decode() if msg else "")


def test_a_null_batch_fails_loudly():
    st, msg = set_solute()
    assert st == _lib.MMC_ERR_ARG and "batch is NULL" in msg
    st, msg = set_solute(n_sites=0, mol=None, charge=None, eps=None, sig=None)   # removing reads no array
    assert st == _lib.MMC_ERR_ARG and "batch is NULL" in msg
    L = _lib.lib()
    assert L.mmc_batch_get_solute(None, None, None, None, None, None) == _lib.MMC_ERR_ARG
    out, ovl = (C.c_double * 4)(), (C.c_uint8 * 4)()
    assert L.mmc_batch_solute_energy(None, out, out, ovl) == _lib.MMC_ERR_ARG
    assert b"batch is NULL" in L.mmc_last_error()
    hist = (C.c_uint64 * 64)()
    assert L.mmc_batch_rdf_solute(None, 4, 0.0, 0, hist) == _lib.MMC_ERR_ARG
    assert b"batch is NULL" in L.mmc_last_error()


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("kw,word", [
    (dict(n_sites=-1), "n_sites"), (dict(n_sites=17), "n_sites"),
    (dict(charge=None), "charge"), (dict(eps=None), "eps"), (dict(sig=None), "sig"), (dict(mol=None), "mol"),
    (dict(charge=(0.4, NAN)), "charge"), (dict(charge=(INF, 0.0)), "charge"),
    (dict(eps=NAN), "eps"), (dict(eps=INF), "eps"), (dict(eps=(1.0, 1.0, 1.0, 1.0, -1e-300, 1.0)), "eps"),
    (dict(sig=NAN), "sig"), (dict(sig=INF), "sig"), (dict(sig=(1.0, 1.0, 1.0, 1.0, 1.0, -3.0)), "sig"),
    (dict(mol=NAN), "mol"), (dict(mol=(0.0,) * 8 + (-INF,)), "mol"),
])
def test_arguments_refused_without_a_device(kw, word):
    st, msg = set_solute(**kw)
    assert st == _lib.MMC_ERR_ARG
    assert word in msg and "batch is NULL" not in msg, msg


@pytest.mark.parametrize("kw,word", [
    # mmc_batch_widom_solute_at's order: n_sites, the NULL arrays charge, eps, sig, mol, then the values
    # charge, eps / sig, mol -- of two bad arguments the earlier one is named
    (dict(n_sites=17, charge=None), "n_sites"), (dict(charge=None, eps=None), "charge"),
    (dict(eps=None, sig=None), "eps"), (dict(sig=None, mol=None), "sig"), (dict(mol=None, charge=(NAN, 0.0)), "NULL mol"),
    (dict(charge=(NAN, 0.0), eps=NAN), "charge"), (dict(eps=-1.0, mol=NAN), "eps"), (dict(sig=-1.0, mol=NAN), "sig"),
])
def test_refusals_come_in_the_documented_order(kw, word):
    st, msg = set_solute(**kw)
    assert st == _lib.MMC_ERR_ARG and word in msg and "batch is NULL" not in msg, msg


def test_the_largest_solute_and_zero_parameters_get_as_far_as_the_batch():
    st, msg = set_solute(S=16, charge=0.0, eps=0.0, sig=0.0, mol=2.0)
    assert st == _lib.MMC_ERR_ARG and "batch is NULL" in msg, msg


@pytest.mark.parametrize("kw,word", [
    (dict(hist=False), "NULL"), (dict(numbins=0), "numbins"), (dict(numbins=2047), "numbins"),
    (dict(r_max=NAN), "r_max"), (dict(r_max=INF), "r_max"),
])
def test_rdf_solute_refuses_what_rdf_sites_refuses_without_a_device(kw, word):
    L = _lib.lib()
    hist = (C.c_uint64 * 64)(*([9] * 64))
    st = L.mmc_batch_rdf_solute(None, kw.get("numbins", 4), kw.get("r_max", 0.0), 0, hist if kw.get("hist", True) else None)
    msg = L.mmc_last_error().decode()
    assert st == _lib.MMC_ERR_ARG and word in msg and "batch is NULL" not in msg, msg
    assert all(v == 9 for v in hist)


def test_solute_energy_refuses_null_outputs_without_a_device():
    L = _lib.lib()
    out, ovl = (C.c_double * 4)(), (C.c_uint8 * 4)()
    for args in ((None, out, ovl), (out, None, ovl), (out, out, None)):
        assert L.mmc_batch_solute_energy(None, *args) == _lib.MMC_ERR_ARG
        msg = L.mmc_last_error().decode()
        assert "NULL out pointer" in msg and "batch is NULL" not in msg, msg
