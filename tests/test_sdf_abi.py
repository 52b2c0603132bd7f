"""CPU tests of mmc_batch_sdf's boundary: declared with the agreed prototype, exported, bound with
matching ctypes, loud on a NULL batch and on every argument that can be refused without a device,
and the Python wrapper's own check of `out`."""
import ctypes as C

import numpy as np
import pytest

import boundary
from boundary import header_define
from common import fake_batch
from metropolismontecarlo_amd import _lib

NAME = "mmc_batch_sdf"
PROTOTYPE = ("int32_t mmc_batch_sdf(mmc_batch *b, int32_t n_half, double cell, int32_t fold, int32_t site_mask, "
             "int32_t per_replica, uint64_t *hist);")
SENTINEL = 0xfedcba9876543210


def test_symbol_is_declared_exported_and_bound_with_the_header_prototype():
    """(Exported and bound with these types: tests/test_abi.py, for every function of the header.)"""
    assert boundary.prototype_text(NAME) == PROTOTYPE


def test_the_header_states_the_definition_and_its_constants():
    src = boundary.header_text()
    sec = src[src.index("Spatial distribution functions"):src.index("int32_t mmc_batch_sdf")]
    assert src.index("Orientational pair correlations") < src.index("Spatial distribution functions") \
        < src.index("Pair-energy distributions")
    for cite in ("dot(a,b) = (a.x b.x + a.y b.y) + a.z b.z", "o1 = vector1D(s0, s1)", "o2 = vector1D(s0, s2)",
                 "boundaries.jl", "b = o1 + o2, h = o2 - o1", "nb2 = dot(b,b), e_z = b / sqrt(nb2)",
                 "t = dot(h, e_z)", "g = h - t e_z (multiply, then subtract)", "ng2 = dot(g,g), e_x = g / sqrt(ng2)",
                 "e_y = e_z x e_x", "e_y.x = e_z.y e_x.z - e_z.z e_x.y", "has no frame when nb2 or ng2 is 0 or not finite",
                 "d = vector1D(s0(i), s0(j))", "-d bit for bit", "w = d + o_a(j)", "w' = -d + o_a(i)",
                 "fold bit 0 replaces p.x by |p.x|", "bit 1 replaces p.y by |p.y|", "z is never folded",
                 "e_k = (double)k * cell", "e_k <= p < e_k+1", "index k + n_half", "k = 0 .. n_half - 1",
                 "a NaN counts\n *     as outside", "(ix g_y + iy) g_z + iz", "g_z = 2 n_half", "then `outside`, then `noframe`",
                 "cells + outside + noframe = N (N - 1) popcount(site_mask) exactly", "\"wave_wgs\"",
                 "hist[R][g_x g_y g_z + 2]", "overwritten, not accumulated", "MMC_ERR_STATE", "MMC_SDF_MAX_CELLS",
                 "sqrt(3) n_half cell + rho <= L_min / 2", "rho = 2 r_mol_max", "tests/sdf_ref.py", "unfused fp64"):
        assert cite in sec, cite
    # 32-bit counters in 128 KB of a workgroup's LDS
    assert int(header_define("MMC_SDF_MAX_CELLS")) == 32768 == 128 * 1024 // 4


def test_the_julia_binding_calls_it():
    assert NAME in boundary.julia_bound()


def call(b=None, n_half=8, cell=0.5, fold=3, site_mask=1, per_replica=0, hist=True):
    h = (C.c_uint64 * 64)(*([SENTINEL] * 64))
    st = _lib.lib().mmc_batch_sdf(b, n_half, cell, fold, site_mask, per_replica, h if hist else None)
    assert all(v == SENTINEL for v in h)
    msg = _lib.lib().mmc_last_error()
    return st, (msg.decode() if msg else "")


def test_a_null_batch_fails_loudly():
    st, msg = call()
    assert st == _lib.MMC_ERR_ARG and "batch is NULL" in msg
    with pytest.raises(_lib.MMCError, match="MMC_ERR_ARG"):
        _lib.check(st)
    # the largest grids of every fold pass the argument checks
    for n_half, fold in ((16, 0), (20, 1), (20, 2), (25, 3)):
        st, msg = call(n_half=n_half, cell=0.1, fold=fold, site_mask=7, per_replica=1)
        assert st == _lib.MMC_ERR_ARG and "batch is NULL" in msg, (n_half, fold)


@pytest.mark.parametrize("kw,word", [
    (dict(hist=False), "NULL out pointer"),
    (dict(n_half=0), "n_half"), (dict(n_half=-3), "n_half"),
    (dict(cell=0.0), "cell"), (dict(cell=-0.5), "cell"), (dict(cell=float("nan")), "cell"),
    (dict(cell=float("inf")), "cell"),
    (dict(fold=-1), "fold"), (dict(fold=4), "fold"),
    (dict(site_mask=0), "site_mask"), (dict(site_mask=8), "site_mask"), (dict(site_mask=-1), "site_mask"),
    (dict(n_half=17, fold=0), "cells"), (dict(n_half=21, fold=1), "cells"), (dict(n_half=21, fold=2), "cells"),
    (dict(n_half=26, fold=3), "cells"), (dict(n_half=2 ** 31 - 1), "cells"),
])
def test_arguments_refused_without_a_device(kw, word):
    """These are refused before the batch is looked at: the message names the argument, not the NULL
    batch, and nothing is written.  (The cube against the boxes needs the batch:
    tests/test_gpu_sdf.py.)"""
    st, msg = call(**kw)
    assert st == _lib.MMC_ERR_ARG
    assert word in msg and "batch is NULL" not in msg, msg


# (device.Batch.sdf's own check of `out` runs before the library is called.)
@pytest.mark.parametrize("kw", [
    dict(out=np.zeros(18, dtype=np.int64)), dict(out=np.zeros(17, dtype=np.uint64)),
    dict(out=np.zeros((2, 18), dtype=np.uint64)), dict(out=np.zeros(36, dtype=np.uint64)[::2]),
    dict(out=[0] * 18), dict(out=np.zeros(18, dtype=np.uint64), per_replica=True),
    dict(out=np.zeros(18, dtype=np.uint64), fold=0), dict(out=np.zeros((2, 2, 8), dtype=np.uint64)),
])
def test_the_wrapper_checks_its_arguments(kw):
    with pytest.raises(ValueError):
        fake_batch("sdf").sdf(2, 0.5, **kw)                 # fold 3: 2 x 2 x 4 cells + 2
    with pytest.raises(AssertionError, match="the library was reached"):
        fake_batch("sdf").sdf(2, 0.5, out=np.zeros(18, dtype=np.uint64))
    with pytest.raises(AssertionError, match="the library was reached"):
        fake_batch("sdf").sdf(2, 0.5, fold=0, per_replica=True, out=np.zeros((2, 66), dtype=np.uint64))
