"""CPU tests of the per-replica-box entry points (mmc_batch_set_boxes and the batched NPT move):
loud on a bad handle without touching a device.  (Declared, exported and bound: tests/test_abi.py.)"""
import ctypes as C

import pytest

from metropolismontecarlo_amd import _lib

def test_per_box_entry_points_fail_loudly_on_a_null_batch():
    L = _lib.lib()
    d = (C.c_double * 4)(30.0, 30.0, 30.0, 30.0)
    acc = (C.c_int32 * 4)()
    tot = (_lib.Totals * 4)()
    p, q, st = _lib.RunParams(), _lib.NptParams(), _lib.RunStats()
    ns = (_lib.NptStats * 4)()
    calls = [lambda: L.mmc_batch_set_boxes(None, d, 5.6),
             lambda: L.mmc_batch_get_boxes(None, d),
             lambda: L.mmc_batch_volume_trial_replicas(None, d, tot),
             lambda: L.mmc_batch_volume_settle(None, acc),
             lambda: L.mmc_batch_run_npt_replicas(None, C.byref(p), C.byref(q), None, d,
                                                  C.byref(st), ns),
             lambda: L.mmc_batch_qq_table_replica(None, 0, d, 1, d)]
    for call in calls:
        status = call()
        assert status != 0
        with pytest.raises(_lib.MMCError, match="MMC_ERR_ARG"):
            _lib.check(status)
