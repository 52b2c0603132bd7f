"""CPU tests of the Wolf-style entry points of the replica batch (mmc_batch_set_coulomb_style,
mmc_batch_get_coulomb_style, mmc_batch_potential_wolf): declared, exported, bound in ctypes and in
MMCHip.jl with the header's arity and types, and loud on a bad handle without touching a device."""
import ctypes as C

import pytest

from metropolismontecarlo_amd import _lib

NEW = ("mmc_batch_set_coulomb_style", "mmc_batch_get_coulomb_style", "mmc_batch_potential_wolf")


def test_wolf_symbols_are_declared_exported_and_bound():
    from test_abi import header_functions
    names = header_functions()
    L = C.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert n in names, n
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES, n
        assert getattr(_lib.lib(), n).argtypes is not None, n


def test_wolf_symbols_are_bound_in_julia_with_the_headers_arity():
    from test_julia_binding import JL, ccall_mismatches, header_prototypes, julia_ccalls
    text = open(JL, encoding="utf-8").read()
    calls = {c[0]: c for c in julia_ccalls(text)}
    protos = header_prototypes()
    for n in NEW:
        assert n in calls, f"{n} is not bound in MMCHip.jl"
        _, ret, types, n_values = calls[n]
        assert ret == "Int32" and len(types) == len(protos[n][1]) == n_values, (n, types, protos[n])
    assert not [m for m in ccall_mismatches(text) if any(n in m for n in NEW)]
    for fn in ("set_coulomb_style!", "coulomb_style", "potential_wolf(b::Batch)"):
        assert fn in text, fn


def test_the_style_constants_are_the_headers():
    from test_julia_binding import HEADER
    src = open(HEADER).read()
    assert "enum { MMC_COULOMB_EWALD = 0, MMC_COULOMB_WOLF = 1 };" in src
    from metropolismontecarlo_amd.device import Batch
    assert Batch.COULOMB_STYLES == ("ewald", "wolf")      # index == the enum's value


def test_wolf_entry_points_fail_loudly_on_a_null_batch():
    L = _lib.lib()
    style = C.c_int32(7)
    tot = (_lib.Totals * 2)()
    calls = [lambda: L.mmc_batch_set_coulomb_style(None, 1),
             lambda: L.mmc_batch_get_coulomb_style(None, C.byref(style)),
             lambda: L.mmc_batch_potential_wolf(None, tot)]
    for call in calls:
        status = call()
        assert status != 0
        with pytest.raises(_lib.MMCError, match="MMC_ERR_ARG"):
            _lib.check(status)
    assert style.value == 7
