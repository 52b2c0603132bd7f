"""CPU tests of mmc_batch_forces' boundary: declared with the agreed prototype, exported, bound with
matching ctypes, loud on a NULL batch and on every argument that can be refused without a device,
and the Python wrapper's own argument checks."""
import ctypes as C

import numpy as np
import pytest

import boundary
from common import fake_batch
from metropolismontecarlo_amd import _lib

NAME = "mmc_batch_forces"
PROTOTYPE = ("int32_t mmc_batch_forces(mmc_batch *b, int32_t n_sel, const int32_t *sel, const double *mass, "
             "double *force_out, double *torque_out, double *vir_out, double *atom_out, double *fsum, "
             "int64_t *n_flagged, uint8_t *ovl_out);")


def test_symbol_is_declared_exported_and_bound_with_the_header_prototype():
    """(Exported and bound with these types: tests/test_abi.py, for every function of the header.)"""
    assert boundary.prototype_text(NAME) == PROTOTYPE


def test_the_header_states_the_definition_with_its_reference_lines():
    src = boundary.header_text()
    sec = src[src.index("Forces and torques on every molecule"):src.index("int32_t mmc_batch_forces")]
    for cite in ("Ewald/energy.jl:946-1032", "energy.jl:254", "ewalds.jl:340", "boundaries.jl:8-14",
                 "energy.jl:270-281", "ewalds.jl:359-367", ":359-360", "ewalds.jl:538-604", ":829-833",
                 "energy.jl:281, :289", "24 eps (2 s12 - s6) / r^2", "2 kappa / sqrt(pi) exp(-kappa^2 r^2)",
                 "factor (4 pi / L) q_a sum_k cfac_k n_k Im(conj(S_k) e_{a,k})", "tau' I^-1 tau",
                 "fsum[r][7] == 2 (virial - coulomb / 3)", "Order of summation within a molecule",
                 "mmc_batch_deletion"):
        assert cite in sec, cite


def test_the_julia_binding_calls_it():
    assert NAME in boundary.julia_bound()


def call(b=None, sel=None, n_sel=0, mass=None, outputs=(True,) * 7):
    force = (C.c_double * 24)(*([7.5] * 24))
    torque = (C.c_double * 24)(*([7.5] * 24))
    vir = (C.c_double * 24)(*([7.5] * 24))
    atom = (C.c_double * 72)(*([7.5] * 72))
    fsum = (C.c_double * 18)(*([7.5] * 18))
    nf = (C.c_int64 * 2)(77, 77)
    ovl = (C.c_uint8 * 8)(*([9] * 8))
    sel_a = None if sel is None else (C.c_int32 * max(len(sel), 1))(*sel)
    mass_a = None if mass is None else (C.c_double * 3)(*mass)
    outs = [x if on else None for x, on in zip((force, torque, vir, atom, fsum, nf, ovl), outputs)]
    st = _lib.lib().mmc_batch_forces(b, n_sel, sel_a, mass_a, *outs)
    for arr in (force, torque, vir, atom, fsum):
        assert all(v == 7.5 for v in arr)
    assert all(v == 77 for v in nf) and all(v == 9 for v in ovl)
    msg = _lib.lib().mmc_last_error()
    return st, (msg.decode() if msg else "")


def test_a_null_batch_fails_loudly():
    st, msg = call()
    assert st == _lib.MMC_ERR_ARG and "NULL" in msg
    with pytest.raises(_lib.MMCError, match="MMC_ERR_ARG"):
        _lib.check(st)
    st, msg = call(mass=(15.9994, 1.00794, 1.00794), sel=[1, 2], n_sel=2)
    assert st == _lib.MMC_ERR_ARG and "batch is NULL" in msg


@pytest.mark.parametrize("kw,word", [
    (dict(outputs=(False,) * 7), "every output is NULL"),
    (dict(sel=[], n_sel=0), "n_sel"), (dict(sel=[3], n_sel=-2), "n_sel"),
    (dict(mass=(0.0, 1.0, 1.0)), "mass[0]"), (dict(mass=(16.0, -1.0, 1.0)), "mass[1]"),
    (dict(mass=(16.0, 1.0, float("nan"))), "mass[2]"), (dict(mass=(float("inf"), 1.0, 1.0)), "mass[0]"),
])
def test_arguments_refused_without_a_device(kw, word):
    """These are refused before the batch is looked at: the message names the argument, not the
    NULL batch, and nothing is written.  (An index outside 0..N-1 needs the batch: tests/
    test_gpu_forces.py.)"""
    st, msg = call(**kw)
    assert st == _lib.MMC_ERR_ARG
    assert word in msg and "batch is NULL" not in msg, msg


# (device.Batch.forces' own argument checks run before the library is called.)
@pytest.mark.parametrize("kw", [
    dict(sel=np.zeros((2, 2), dtype=np.int64)), dict(sel=np.array([0.5, 1.0])), dict(sel=np.array([2 ** 40])),
    dict(mass=np.ones(2)), dict(mass=np.ones((3, 1))),
    dict(n_flagged=np.zeros(2)), dict(n_flagged=np.zeros(4, dtype=np.int64)[::2]), dict(n_flagged=[0, 0]),
])
def test_the_wrapper_checks_its_arguments(kw):
    with pytest.raises(ValueError):
        fake_batch("forces").forces(**kw)
