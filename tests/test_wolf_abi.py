"""CPU tests of the Wolf-style entry points of the replica batch (mmc_batch_set_coulomb_style,
mmc_batch_get_coulomb_style, mmc_batch_potential_wolf): declared, exported, bound in ctypes and in
MMCHip.jl with the header's arity and types, and loud on a bad handle without touching a device."""
import ctypes as C

import pytest

import boundary
from metropolismontecarlo_amd import _lib

NEW = ("mmc_batch_set_coulomb_style", "mmc_batch_get_coulomb_style", "mmc_batch_potential_wolf")


def test_wolf_symbols_are_bound_in_julia_with_the_headers_arity():
    """(With the header's arity and types: tests/test_julia_binding.py, for every ccall.)"""
    assert set(NEW) <= boundary.julia_bound()
    text = boundary.julia_text()
    for fn in ("set_coulomb_style!", "coulomb_style", "potential_wolf(b::Batch)"):
        assert fn in text, fn


def test_the_style_constants_are_the_headers():
    src = boundary.header_text()
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
