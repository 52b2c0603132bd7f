"""CPU tests of mmc_batch_hydration_map's boundary: declared with the agreed prototype and constants,
bound by ctypes and by the Julia module, loud on a NULL batch and on every argument that is refused
without a device, in the stated order, with the output left alone; and the Python wrapper's own checks."""
import ctypes as C

import numpy as np
import pytest

import boundary
from boundary import header_define
from common import fake_batch
from metropolismontecarlo_amd import _lib
from metropolismontecarlo_amd.device import Batch

NAME = "mmc_batch_hydration_map"
PROTOTYPE = ("int32_t mmc_batch_hydration_map(mmc_batch *b, int32_t n_half, double cell, int32_t channel_mask, "
             "int32_t per_replica, int64_t *maps);")
SENTINEL = -0x0123456789abcdef


def test_symbol_is_declared_and_bound_with_the_header_prototype():
    """(Exported and bound with these types: tests/test_abi.py, for every function of the header.)"""
    assert boundary.prototype_text(NAME) == PROTOTYPE
    assert _lib.SIGNATURES[NAME] == boundary.bound_argtypes(NAME)
    assert hasattr(_lib.lib(), NAME)


def test_the_header_defines_the_constants_and_states_the_definition():
    assert int(header_define("MMC_HMAP_CHANNELS")) == 8
    assert int(header_define("MMC_HMAP_MAX_CELLS")) == 16384 == 128 * 1024 // 8 and 24 ** 3 <= 16384 < 26 ** 3
    assert float(header_define("MMC_HMAP_VEC_SCALE")) == 2.0 ** 30
    assert float(header_define("MMC_HMAP_E_SCALE")) == 2.0 ** 20 == float(header_define("MMC_PAIRE_SCALE"))
    src = boundary.header_text()
    sec = src[src.index("A fixed solute"):src.index("int32_t mmc_batch_hydration_map")]
    for cite in ("e_k = (double)k * cell", "e_k <= p < e_k+1", "index k + n_half", "(ix g + iy) g + iz", "g = 2 n_half",
                 "a NaN counts as outside", "x = w - c", "|x| > L / 2 (strict)", "o_a = vector1D(s0, s_a)", "b = o1 + o2",
                 "nb2 = dot(b,b)", "sqrt(nb2)", "ties to even", "u_lj = (0.0 + sum_lj) * 4", "u_real = factor * (0.0 +",
                 "magnitude >= 2^20 K", "modulo 2^64", "\"wave_wgs\"", "overwritten, not accumulated", "unfused fp64",
                 "IEEE sqrt and divide", "popcount(channel_mask)", "rising bit order", "(double)n_half * cell > L / 2",
                 "allocation's status", "tests/hydration_map_ref.py"):
        assert cite in sec, cite


def test_the_julia_binding_and_the_python_class_have_it():
    assert NAME in boundary.julia_bound()
    assert callable(getattr(Batch, "hydration_map"))
    assert Batch.HYDRATION_CHANNELS == ("O", "H1", "H2", "px", "py", "pz", "u_lj", "u_real")


def call(b=None, n_half=8, cell=0.5, channel_mask=255, per_replica=0, maps=True):
    h = (C.c_int64 * 64)(*([SENTINEL] * 64))
    st = _lib.lib().mmc_batch_hydration_map(b, n_half, cell, channel_mask, per_replica, h if maps else None)
    assert all(v == SENTINEL for v in h)
    msg = _lib.lib().mmc_last_error()
    return st, (msg.decode() if msg else "")


def test_a_null_batch_fails_loudly():
    st, msg = call()
    assert st == _lib.MMC_ERR_ARG and "batch is NULL" in msg
    with pytest.raises(_lib.MMCError, match="MMC_ERR_ARG"):
        _lib.check(st)
    for kw in (dict(n_half=12, cell=1e-300, channel_mask=1, per_replica=1), dict(n_half=1, cell=1e300, channel_mask=128)):
        st, msg = call(**kw)                         # the extremes of every argument pass the argument checks
        assert st == _lib.MMC_ERR_ARG and "batch is NULL" in msg, kw


# in the order of the checks: each case is bad in its own argument and in every later one
ORDER = [(dict(maps=False), "NULL out pointer"), (dict(n_half=0), "n_half"), (dict(cell=float("nan")), "cell"),
         (dict(channel_mask=0), "channel_mask"), (dict(n_half=13), "cells")]


@pytest.mark.parametrize("first", range(len(ORDER)))
def test_arguments_are_refused_in_the_stated_order(first):
    kw = {}
    for later, _ in ORDER[first + 1:][::-1]:
        kw.update(later)
    kw.update(ORDER[first][0])
    st, msg = call(**kw)
    assert st == _lib.MMC_ERR_ARG and ORDER[first][1] in msg and "batch is NULL" not in msg, msg


@pytest.mark.parametrize("kw,word", [
    (dict(maps=False), "NULL out pointer"),
    (dict(n_half=0), "n_half"), (dict(n_half=-3), "n_half"),
    (dict(cell=0.0), "cell"), (dict(cell=-0.5), "cell"), (dict(cell=float("nan")), "cell"), (dict(cell=float("inf")), "cell"),
    (dict(channel_mask=0), "channel_mask"), (dict(channel_mask=256), "channel_mask"), (dict(channel_mask=-1), "channel_mask"),
    (dict(n_half=13), "cells"), (dict(n_half=2 ** 31 - 1), "cells"), (dict(n_half=46341), "cells"),
])
def test_arguments_refused_without_a_device(kw, word):
    """Refused before the batch is looked at: the message names the argument, not the NULL batch, and
    nothing is written.  (The cube against the box needs the batch: tests/test_gpu_hydration_map.py.)"""
    st, msg = call(**kw)
    assert st == _lib.MMC_ERR_ARG
    assert word in msg and "batch is NULL" not in msg, msg


@pytest.mark.parametrize("kw", [
    dict(out=np.zeros((8, 66), dtype=np.uint64)), dict(out=np.zeros((8, 65), dtype=np.int64)),
    dict(out=np.zeros((7, 66), dtype=np.int64)), dict(out=np.zeros((2, 8, 66), dtype=np.int64)),
    dict(out=np.zeros((8, 132), dtype=np.int64)[:, ::2]), dict(out=[[0] * 66] * 8),
    dict(out=np.zeros((8, 66), dtype=np.int64), per_replica=True), dict(out=np.zeros((8, 66), dtype=np.int64), channels=127),
    dict(channels=("O", "water")), dict(channels="H3"),
])
def test_the_wrapper_checks_its_arguments(kw):
    with pytest.raises(ValueError):
        fake_batch("hydration_map", HYDRATION_CHANNELS=Batch.HYDRATION_CHANNELS).hydration_map(2, 0.5, **kw)


def test_the_wrapper_turns_names_into_the_mask():
    seen = []

    class Lib:
        def mmc_batch_hydration_map(self, h, n_half, cell, mask, per_replica, maps):
            seen.append((n_half, cell, mask, per_replica))
            return 0
    fb = fake_batch("hydration_map", _L=Lib(), HYDRATION_CHANNELS=Batch.HYDRATION_CHANNELS)
    assert fb.hydration_map(2, 0.5).shape == (8, 66) and fb.hydration_map(1, 0.5, per_replica=True).shape == (2, 8, 10)
    assert fb.hydration_map(2, 0.5, channels=("u_real", "O", "pz", "O")).shape == (3, 66)
    assert fb.hydration_map(2, 0.5, channels="H2").shape == (1, 66)
    assert fb.hydration_map(2, 0.5, channels=0b1010, out=np.ones((2, 66), dtype=np.int64)).sum() == 132
    assert seen == [(2, 0.5, 255, 0), (1, 0.5, 255, 1), (2, 0.5, 0b10100001, 0), (2, 0.5, 4, 0), (2, 0.5, 10, 0)]
