"""CPU tests of mmc_batch_solute_forces' boundary: declared with the agreed prototype, bound by ctypes and by
the Julia module with the header's types, loud on a NULL batch and on a call without outputs, with the
outputs left alone; the header states the definitions; and the Python wrapper's own checks."""
import ctypes as C

import numpy as np
import pytest

import boundary
from common import fake_batch
from metropolismontecarlo_amd import _lib, observables
from metropolismontecarlo_amd.device import Batch

NAME = "mmc_batch_solute_forces"
PROTOTYPE = ("int32_t mmc_batch_solute_forces(mmc_batch *b, double *force_out, double *torque_out, double *site_lj_out, "
             "double *field_out, double *phi_out, double *recip_out, uint8_t *flags_out);")
SENTINEL = -1.2345e300


def test_symbol_is_declared_and_bound_with_the_header_prototype():
    assert boundary.prototype_text(NAME) == PROTOTYPE
    assert _lib.SIGNATURES[NAME] == boundary.bound_argtypes(NAME)
    assert hasattr(_lib.lib(), NAME)


def test_the_julia_binding_and_the_python_layers_have_it():
    assert NAME in boundary.julia_bound()
    assert callable(getattr(Batch, "solute_forces"))
    for f in ("solute_mean_force", "pair_mean_force", "pmf_from_mean_force", "charging_derivative", "charging_free_energy"):
        assert callable(getattr(observables, f))
    assert "no intramolecular term" in observables.pmf_from_mean_force.__doc__


def test_the_header_states_the_definitions():
    src = boundary.header_text()
    sec = src[src.index("the mean force, field and potential on it"):src.index("int32_t mmc_batch_solute_forces")]
    for cite in ("energy.jl:946-1032", "energy.jl:209-290", "ewalds.jl:892-906", "EwaldReal :293-376", "ewalds.jl:538-602", "ewalds.jl:829-833", "ewalds.jl:564-585",
                 "WHETHER OR NOT the solute is charged", "rab = vector1D(atom b, site a)",
                 "site_lj[a] += 24 eps_ab (2 s12 - s6) / u * rab",
                 "field[a] += factor q_b (erfc(kappa r) / r + 2 kappa / sqrt(pi) exp(-kappa^2 u)) / u * rab",
                 "phi[a]   += factor q_b erfc(kappa r) / r",
                 "field[a] += factor (4 pi / L) sum_k cfac_k n_k Im(conj(S_k) e_{a,k})",
                 "phi[a]   += 2 factor sum_k cfac_k Re(conj(S_k) e_{a,k})", "phi[a]   -= 2 factor kappa / sqrt(pi) q_a",
                 "phi[a] = dU/dq_a", "f_a = site_lj[a] + q_a field[a] = -dU/dr_a", "d_a = vector1D(c, r_a)",
                 "tau = sum_a d_a x f_a", "zeros in every row", "l, l + 64", "\"wave_wgs\"", "every output is\n *   untouched",
                 "tests/solute_force_ref.py"):
        assert cite in sec, cite


def call(b=None, which=range(7)):
    """The call with the outputs `which` given (sentinel arrays of 64 entries), the others NULL."""
    f = [(C.c_double * 64)(*([SENTINEL] * 64)) for _ in range(6)]
    fl = (C.c_uint8 * 64)(*([0xA5] * 64))
    args = [f[k] if k in which else None for k in range(6)] + [fl if 6 in which else None]
    st = _lib.lib().mmc_batch_solute_forces(b, *args)
    assert all(v == SENTINEL for a in f for v in a) and all(v == 0xA5 for v in fl)
    msg = _lib.lib().mmc_last_error()
    return st, (msg.decode() if msg else "")


def test_a_null_batch_fails_loudly():
    for which in (range(7), (0,), (6,), (2, 4)):
        st, msg = call(which=which)
        assert st == _lib.MMC_ERR_ARG and "batch is NULL" in msg
    with pytest.raises(_lib.MMCError, match="MMC_ERR_ARG"):
        _lib.check(st)


def test_a_call_without_outputs_is_refused_before_the_batch_is_looked_at():
    st, msg = call(which=())
    assert st == _lib.MMC_ERR_ARG and "every output is NULL" in msg and "batch is NULL" not in msg


class Lib:
    def __init__(self):
        self.seen = []

    def mmc_batch_solute_forces(self, h, *ptrs):
        self.seen.append([p is not None for p in ptrs])
        return 0


def fake(S=2):
    return fake_batch("solute_forces", _L=Lib(), _solute_sites=lambda: S)


def test_the_wrapper_passes_the_outputs_it_was_asked_for():
    fb = fake()
    res = fb.solute_forces()
    assert list(res) == ["force", "torque", "flags"] and res["force"].shape == (fb.R, 3) and res["flags"].dtype == np.uint8
    res = fb.solute_forces(details=True)
    assert list(res) == ["force", "torque", "site_lj", "field", "phi", "recip", "flags"]
    assert res["site_lj"].shape == (fb.R, 2, 3) == res["field"].shape and res["phi"].shape == (fb.R, 2)
    assert res["recip"].shape == (fb.R, 2, 4)
    assert fb._L.seen == [[True, True, False, False, False, False, True], [True] * 7]
    mine = np.ones((fb.R, 3))
    assert fb.solute_forces(out={"torque": mine})["torque"] is mine


@pytest.mark.parametrize("kw", [
    dict(out={"force": np.zeros((1, 3))}), dict(out={"phi": np.zeros((2, 2))}), dict(out=[np.zeros((2, 3))]),
    dict(out={"flags": np.zeros(2, dtype=np.int32)}), dict(details=True, out={"recip": np.zeros((2, 2, 3))}),
    dict(details=True, out={"field": np.zeros((2, 2, 6))[:, :, ::2]}),
])
def test_the_wrapper_checks_its_arguments(kw):
    with pytest.raises(ValueError):
        fake().solute_forces(**kw)
