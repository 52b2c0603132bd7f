"""CPU tests of the parallel-tempering entry points (mmc_batch_set_temperatures,
mmc_batch_get_temperatures, mmc_exchange_round, mmc_batch_exchange, mmc_batch_run_exchange):
declared, exported, bound in ctypes and in MMCHip.jl with the header's arity and types, and loud on
a bad handle without touching a device."""
import ctypes as C

import numpy as np
import pytest

import boundary
from metropolismontecarlo_amd import _lib

NEW = ("mmc_batch_set_temperatures", "mmc_batch_get_temperatures", "mmc_exchange_round", "mmc_batch_exchange",
       "mmc_batch_run_exchange")


def test_tempering_symbols_are_bound_in_julia_with_the_headers_arity():
    """(With the header's arity and types: tests/test_julia_binding.py, for every ccall.)"""
    assert set(NEW) <= boundary.julia_bound()
    text = boundary.julia_text()
    for fn in ("set_temperatures!", "exchange!(b::Batch", "run_exchange!(b::Batch"):
        assert fn in text, fn


def test_the_exchange_slot_is_the_headers_and_the_restatements():
    import tempering_ref
    assert "#define MMC_SLOT_EXCHANGE 0x60000000u" in boundary.header_text()
    assert tempering_ref.SLOT_EXCHANGE == 0x60000000


def test_batch_entry_points_fail_loudly_on_a_null_batch():
    L = _lib.lib()
    t = np.full(4, 300.0)
    e, rung = np.zeros(4), np.array([0, 1, 0, 1], dtype=np.int32)
    att, acc = np.zeros(1, np.int64), np.zeros(1, np.int64)
    p, st = _lib.RunParams(300.0, 0.1, 0.1, 1, 4, 1, 0, 0, 1, 0, 0, 0), _lib.RunStats()
    dp, ip, lp = _lib._dp, _lib._i32p, _lib._i64p
    calls = [lambda: L.mmc_batch_set_temperatures(None, t.ctypes.data_as(dp)),
             lambda: L.mmc_batch_get_temperatures(None, t.ctypes.data_as(dp)),
             lambda: L.mmc_batch_exchange(None, 2, 0, 1, 0, 0, 0.0, e.ctypes.data_as(dp), rung.ctypes.data_as(ip),
                                          att.ctypes.data_as(lp), acc.ctypes.data_as(lp)),
             lambda: L.mmc_batch_run_exchange(None, C.byref(p), 1, 2, 0, e.ctypes.data_as(dp), rung.ctypes.data_as(ip),
                                              att.ctypes.data_as(lp), acc.ctypes.data_as(lp), C.byref(st))]
    for call in calls:
        status = call()
        assert status != 0
        with pytest.raises(_lib.MMCError, match="MMC_ERR_ARG"):
            _lib.check(status)
    assert (t == 300.0).all() and rung.tolist() == [0, 1, 0, 1] and att[0] == 0 and acc[0] == 0


def test_exchange_round_needs_no_device_and_refuses_null_arrays():
    """The pure function runs where there is no GPU, and a NULL array (other than volumes) is
    MMC_ERR_ARG."""
    L = _lib.lib()
    t, e = np.array([250.0, 300.0]), np.array([-10.0, -500.0])        # D > 0: certain swap
    rung, att, acc = np.array([0, 1], dtype=np.int32), np.zeros(1, np.int64), np.zeros(1, np.int64)
    dp, ip, lp = _lib._dp, _lib._i32p, _lib._i64p
    assert L.mmc_exchange_round(1, 2, 0, 9, 0, 0, 0.0, e.ctypes.data_as(dp), None, t.ctypes.data_as(dp),
                                rung.ctypes.data_as(ip), att.ctypes.data_as(lp), acc.ctypes.data_as(lp)) == 0
    assert t.tolist() == [300.0, 250.0] and rung.tolist() == [1, 0] and att[0] == 1 and acc[0] == 1
    status = L.mmc_exchange_round(1, 2, 0, 9, 0, 0, 0.0, None, None, t.ctypes.data_as(dp), rung.ctypes.data_as(ip),
                                  att.ctypes.data_as(lp), acc.ctypes.data_as(lp))
    with pytest.raises(_lib.MMCError, match="MMC_ERR_ARG"):
        _lib.check(status)
