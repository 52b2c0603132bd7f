"""CPU tests of mmc_batch_hbond_rings' boundary: declared with the agreed prototype, exported, bound
with matching ctypes, and loud on a NULL batch and on every argument that can be refused without a
device."""
import ctypes as C
import math
import re

import pytest

import boundary
from metropolismontecarlo_amd import _lib

NAME = "mmc_batch_hbond_rings"
PROTOTYPE = ("int32_t mmc_batch_hbond_rings(mmc_batch *b, double r_hb, double cos_hb, int32_t n_max, "
             "int32_t per_replica, uint64_t *ring_hist, uint64_t *member_hist, int64_t *stats, "
             "uint16_t *count_out, int64_t max_rings, int32_t *ring_out);")
COS30 = math.cos(math.radians(30.0))
N = 40   # the size the untouched outputs are laid out for


def test_symbol_is_declared_exported_and_bound_with_the_header_prototype():
    """(Exported and bound with these types: tests/test_abi.py, for every function of the header.)"""
    assert boundary.prototype_text(NAME) == PROTOTYPE


def test_the_header_states_the_limits_and_the_definitions():
    text = boundary.header_text()
    for name, value in (("MMC_RING_MAX_SIZE", 8), ("MMC_RING_MAX_DEG", 8), ("MMC_RING_STATS", 8),
                        ("MMC_RING_MEMBER_BINS", 33)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
    m = re.search(r"#define\s+MMC_NET_MAX_MOL\s+(\d+)", text)
    assert m and int(m.group(1)) >= 2048
    for word in ("Franzblau", "Matsumoto, Baba and Ohmine", "tests/rings_ref.py", "The reference has no such analysis",
                 "min(|a - b|, n - |a - b|)", "Homodromic", "ring_chunk"):
        assert word in text, word


def call(b=None, r_hb=3.5, cos_hb=COS30, n_max=8, outputs=(True, True, True), max_rings=4, ring=True):
    rh = (C.c_uint64 * 27)(*([77] * 27))
    mh = (C.c_uint64 * (9 * 33))(*([77] * (9 * 33)))
    st = (C.c_int64 * 16)(*([-7] * 16))
    cn = (C.c_uint16 * (2 * N * 9))(*([5] * (2 * N * 9)))
    rg = (C.c_int32 * (2 * 4 * 8))(*([-5] * (2 * 4 * 8)))
    status = _lib.lib().mmc_batch_hbond_rings(b, r_hb, cos_hb, n_max, 0, rh if outputs[0] else None,
                                              mh if outputs[1] else None, st if outputs[2] else None, cn, max_rings,
                                              rg if ring else None)
    assert all(v == 77 for v in rh) and all(v == 77 for v in mh) and all(v == -7 for v in st)
    assert all(v == 5 for v in cn) and all(v == -5 for v in rg)
    msg = _lib.lib().mmc_last_error()
    return status, (msg.decode() if msg else "")


def test_a_null_batch_fails_loudly():
    st, msg = call()
    assert st == _lib.MMC_ERR_ARG and "NULL" in msg
    with pytest.raises(_lib.MMCError, match="MMC_ERR_ARG"):
        _lib.check(st)
    for kw in (dict(n_max=3, cos_hb=1.0, max_rings=1), dict(n_max=8, max_rings=0, ring=False),
               dict(max_rings=-5, ring=False), dict(outputs=(False, False, True)), dict(outputs=(True, False, False))):
        st, msg = call(**kw)                                   # the edges of every range pass
        assert st == _lib.MMC_ERR_ARG and "batch is NULL" in msg, kw


@pytest.mark.parametrize("kw,word", [
    (dict(r_hb=float("nan")), "r_hb"), (dict(r_hb=float("inf")), "r_hb"), (dict(r_hb=0.0), "r_hb"), (dict(r_hb=-3.5), "r_hb"),
    (dict(cos_hb=0.0), "cos_hb"), (dict(cos_hb=-0.5), "cos_hb"), (dict(cos_hb=math.nextafter(1.0, 2.0)), "cos_hb"),
    (dict(cos_hb=float("nan")), "cos_hb"),
    (dict(n_max=2), "n_max"), (dict(n_max=9), "n_max"), (dict(n_max=0), "n_max"), (dict(n_max=-8), "n_max"),
    (dict(outputs=(False, False, False)), "at least one"),
    (dict(max_rings=0), "max_rings"), (dict(max_rings=-1), "max_rings"),
])
def test_arguments_refused_without_a_device(kw, word):
    """These are refused before the batch is looked at: the message names the argument, not the
    NULL batch, and nothing is written."""
    st, msg = call(**kw)
    assert st == _lib.MMC_ERR_ARG
    assert word in msg and "batch is NULL" not in msg, msg


def test_the_julia_method_passes_the_prototypes_types():
    """boundary.julia_ccalls reads the ccall(...) form and boundary.C2J knows no 16-bit pointer; this
    method is written with the @ccall macro, so its argument types are held against the prototype here."""
    text = re.sub(r"(?m)#[^\n]*$", "", boundary.julia_text())
    m = re.search(r"@ccall libmmc\.%s\((.*?)\)::Int32\)" % NAME, text, flags=re.S)
    assert m, "MMCHip.jl does not call " + NAME
    types = re.findall(r"::((?:Ptr\{\w+\})|\w+)\s*(?:,|$)", re.sub(r"\s+", " ", m.group(1)))
    julia = dict(boundary.C2J, **{"uint16_t*": "Ptr{UInt16}"})
    assert types == [julia[c] for c in boundary.header_prototypes()[NAME][1]]
    assert re.search(r"(?m)^function hbond_rings\(b::Batch;", text)
