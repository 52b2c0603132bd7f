"""CPU tests of save and resume: the record layout (the library's pure host function against its
Python mirror), the checkpoint file (round trip, refusals that name what is wrong, atomicity) and
Batch.load's refusal of another system's checkpoint before it reaches the library."""
import os
import struct

import numpy as np
import pytest

import common
from metropolismontecarlo_amd import _lib, checkpoint

N_MOL = (1, 2, 100, 750)
NKVECS = (293, 337)


def make_info(n_mol=7, nkvecs=293, quat_mode=0, R=6, **kw):
    d = dict(magic=checkpoint.STATE_MAGIC, version=checkpoint.STATE_VERSION, R=R, n_mol=n_mol, nkvecs=nkvecs,
             half_k=int(nkvecs == 293), lj_rcut=10.0, qq_rcut=10.0, topology=0x0123456789ABCDEF ^ (1 << 63), nk=5,
             k_sq_max=27, factor=167101.00149, coulomb_style=0, s_stale=0, per_box=0, alpha=0.0, temps_on=1,
             quat_mode=quat_mode, db=[0.1 * k for k in range(9)], box=20.0, kappa=0.28, steps_done=12345,
             r_mol_max=float("inf"), rigid_only=1)
    d.update(kw)
    return d


@pytest.mark.parametrize("quat_mode", (0, 1, 2))
@pytest.mark.parametrize("nkvecs", NKVECS)
@pytest.mark.parametrize("n_mol", N_MOL)
def test_record_layout_of_the_library_and_its_python_mirror(n_mol, nkvecs, quat_mode):
    info = make_info(n_mol, nkvecs, quat_mode)
    off, rb = checkpoint.record_layout(info)
    assert (off, rb) == checkpoint.library_layout(info)
    assert all(b > a for a, b in zip(off[:6], off[1:7])) and off[7] >= off[6]       # the offsets ascend
    assert (off[7] > off[6]) == (quat_mode != 0)
    assert all(o % 8 == 0 for o in off) and all(o % 16 == 0 for o in off[3:])
    assert rb % 64 == 0 and off[7] <= rb < off[7] + 64
    # every section holds what the header says it does
    assert off[1] - off[0] >= 8 and off[2] - off[1] >= 8 and off[3] - off[2] >= 8
    assert off[4] - off[3] >= 24 * n_mol and off[5] - off[4] >= 72 * n_mol and off[6] - off[5] >= 16 * nkvecs
    assert off[7] - off[6] == (32 * n_mol if quat_mode else 0)


@pytest.mark.parametrize("quat_mode", (0, 1, 2))
@pytest.mark.parametrize("nkvecs", NKVECS)
def test_record_layout_at_every_size_up_to_three_slabs(nkvecs, quat_mode):
    """Every n_mol of 1..260 (odd and even, both sides of the slab edges 128 and 256 of the state
    kernels): the two implementations agree and the offsets obey the rules of state_layout --
    sections start on 16 bytes, a section of an odd number of doubles (com 3 n, coords 9 n: odd
    exactly when n is) is followed by a pad of exactly 8 bytes and every other by none, the record
    ends on the next multiple of 64."""
    for n in range(1, 261):
        info = make_info(n, nkvecs, quat_mode)
        off, rb = checkpoint.record_layout(info)
        assert (off, rb) == checkpoint.library_layout(info), n
        assert off[:4] == [0, 8, 16, 32], n                              # box, temperature, flags and 8 zero bytes
        assert all(o % 16 == 0 for o in off[3:]), (n, off)
        pad = 8 * (n % 2)
        assert off[4] - (off[3] + 24 * n) == pad and off[5] - (off[4] + 72 * n) == pad, (n, off)
        assert off[6] == off[5] + 16 * nkvecs, (n, off)                  # (16 bytes an entry: never padded)
        assert off[7] == off[6] + (32 * n if quat_mode else 0), (n, off)
        assert rb % 64 == 0 and off[7] <= rb < off[7] + 64, (n, off, rb)


def test_the_library_refuses_an_info_that_is_not_one():
    with pytest.raises(_lib.MMCError, match="MMC_ERR_ARG.*version"):
        checkpoint.library_layout(make_info(version=2))
    with pytest.raises(_lib.MMCError, match="MMC_ERR_ARG"):
        checkpoint.library_layout(make_info(n_mol=0))


def test_state_info_mirror_has_the_headers_layout(tmp_path):
    import ctypes as C
    import subprocess
    from boundary import HEADER
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mmc_hip.h"\nint main(void){\n'
                    'printf("%zu %zu %zu %zu %zu\\n", sizeof(mmc_state_info), offsetof(mmc_state_info, topology), '
                    'offsetof(mmc_state_info, db), offsetof(mmc_state_info, steps_done), offsetof(mmc_state_info, reserved));\n'
                    "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(prog), "-o", str(exe)])
    got = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    S = _lib.StateInfo
    assert got == [C.sizeof(S), S.topology.offset, S.db.offset, S.steps_done.offset, S.reserved.offset]
    assert C.sizeof(S) == 8 * 42
    assert hex(checkpoint.STATE_MAGIC) == common.header_define("MMC_STATE_MAGIC").lower().rstrip("ul")
    assert str(checkpoint.STATE_VERSION) == common.header_define("MMC_STATE_VERSION")


# ---- the file ---------------------------------------------------------------------------------------
def synthetic(info, seed=3):
    """Records of info["R"] replicas with every section filled with its own random doubles."""
    rng = np.random.default_rng(seed)
    off, rb = checkpoint.record_layout(info)
    R, n, nk = info["R"], info["n_mol"], info["nkvecs"]
    rec = np.zeros((R, rb), dtype=np.uint8)
    parts = []
    for r in range(R):
        p = dict(box=20.0 + r, temperature=300.0 + r, flags=2 | (4 if info["quat_mode"] else 0),
                 com=rng.normal(size=(n, 3)), coords=rng.normal(size=(3 * n, 3)),
                 S=rng.normal(size=nk) + 1j * rng.normal(size=nk),
                 quat=rng.normal(size=(n, 4)) if info["quat_mode"] else None)
        rec[r, off[0]:off[0] + 8] = np.array([p["box"]]).view(np.uint8)
        rec[r, off[1]:off[1] + 8] = np.array([p["temperature"]]).view(np.uint8)
        rec[r, off[2]:off[2] + 8] = np.array([p["flags"]], dtype=np.uint64).view(np.uint8)
        for k, name in ((3, "com"), (4, "coords"), (5, "S"), (6, "quat")):
            if p[name] is not None:
                raw = np.ascontiguousarray(p[name]).view(np.uint8).ravel()
                rec[r, off[k]:off[k] + raw.shape[0]] = raw
        parts.append(p)
    return rec, parts


def synthetic_extra(R):
    rng = np.random.default_rng(11)
    chains = np.zeros(R, dtype=_lib.CHAIN_DTYPE)
    for name in _lib.CHAIN_DTYPE.names:
        chains[name] = rng.integers(1, 1000, size=R) if _lib.CHAIN_DTYPE[name].kind == "i" else rng.normal(size=R)
    return dict(energies=rng.normal(size=R), chains=chains, rung=rng.permutation(R).astype(np.int32),
                attempt=np.arange(5, dtype=np.int64), accept=np.arange(5, dtype=np.int64) // 2,
                round=np.array(17, dtype=np.int64), npt=rng.normal(size=(R, 3)))


def write_synthetic(path, info, rec, extra, chunk_records=4, **kw):
    checkpoint.write(str(path), info, info["R"], lambda r0, n: np.ascontiguousarray(rec[r0:r0 + n]), extra=extra,
                     replica0=1000, chunk_records=chunk_records, **kw)


@pytest.mark.parametrize("quat_mode", (0, 2))
def test_file_round_trip(tmp_path, quat_mode):
    info = make_info(quat_mode=quat_mode, R=10)
    rec, parts = synthetic(info)
    extra = synthetic_extra(info["R"])
    path = tmp_path / "a.ckpt"
    write_synthetic(path, info, rec, extra)                   # chunks of 4, 4 and a ragged 2
    assert not os.path.exists(str(path) + ".tmp")
    head = checkpoint.read_header(str(path))
    assert head["info"] == info and head["replica0"] == 1000 and head["n_records"] == 10
    assert len(head["chunk_crc32"]) == 3 and head["record_bytes"] == rec.shape[1]
    assert checkpoint.info_to_dict(checkpoint.info_from_dict(head["info"])) == info      # through the C struct, exactly
    for r in (0, 3, 4, 9):
        got = checkpoint.read_replica(str(path), r)
        for k, want in parts[r].items():
            if want is None:
                assert got[k] is None
            elif isinstance(want, np.ndarray):
                assert got[k].dtype == want.dtype and got[k].shape == want.shape
                assert got[k].tobytes() == want.tobytes(), (r, k)
            else:
                assert got[k] == want, (r, k)
    back = np.concatenate([c for _, c in checkpoint.iter_chunks(str(path))])
    assert back.tobytes() == rec.tobytes()
    got = checkpoint.read_extra(str(path))
    assert sorted(got) == sorted(extra)
    for k, want in extra.items():
        assert got[k].dtype == want.dtype and got[k].shape == want.shape and got[k].tobytes() == want.tobytes(), k
    assert got["chains"].dtype == _lib.CHAIN_DTYPE
    for name in _lib.CHAIN_DTYPE.names:
        assert (got["chains"][name] == extra["chains"][name]).all()
    boxes, temps = checkpoint.verify(str(path))
    assert boxes.tolist() == [p["box"] for p in parts] and temps.tolist() == [p["temperature"] for p in parts]


@pytest.fixture
def good(tmp_path):
    info = make_info(R=10)
    rec, _ = synthetic(info)
    path = tmp_path / "good.ckpt"
    write_synthetic(path, info, rec, synthetic_extra(10))
    return str(path), info, rec


def test_one_flipped_byte_in_a_record_chunk_is_named(good, tmp_path):
    path, info, rec = good
    head = checkpoint.read_header(path)
    raw = bytearray(open(path, "rb").read())
    first = head["data_offset"] + head["extra_bytes"]
    for chunk, r in ((0, 1), (1, 6), (2, 9)):
        bad = bytearray(raw)
        bad[first + r * rec.shape[1] + 40] ^= 0x10
        p = str(tmp_path / f"flip{chunk}.ckpt")
        open(p, "wb").write(bad)
        checkpoint.read_header(p)                                       # the header is fine
        with pytest.raises(checkpoint.CheckpointError, match=f"CRC mismatch in record chunk {chunk}"):
            checkpoint.verify(p)
        with pytest.raises(checkpoint.CheckpointError, match=f"CRC mismatch in record chunk {chunk}"):
            checkpoint.read_replica(p, r)
    bad = bytearray(raw)
    bad[head["data_offset"] + head["extra"]["rung"]["offset"]] ^= 1
    p = str(tmp_path / "flipx.ckpt")
    open(p, "wb").write(bad)
    with pytest.raises(checkpoint.CheckpointError, match="CRC mismatch in extra array 'rung'"):
        checkpoint.read_extra(p)


def test_a_cut_file_is_refused_as_truncated(good, tmp_path):
    path, info, rec = good
    raw = open(path, "rb").read()
    head = checkpoint.read_header(path)
    for n in (0, 7, 19, 21, head["data_offset"] - 1, head["data_offset"], head["data_offset"] + head["extra_bytes"] + 5,
              len(raw) - rec.shape[1], len(raw) - 1):
        p = str(tmp_path / f"cut{n}.ckpt")
        open(p, "wb").write(raw[:n])
        with pytest.raises(checkpoint.CheckpointError, match="truncated"):
            checkpoint.read_header(p)
    p = str(tmp_path / "long.ckpt")
    open(p, "wb").write(raw + b"\0")
    with pytest.raises(checkpoint.CheckpointError, match="beyond the end"):
        checkpoint.read_header(p)


def test_wrong_magic_and_version_are_named(good, tmp_path):
    path, info, rec = good
    raw = open(path, "rb").read()
    p = str(tmp_path / "magic.ckpt")
    open(p, "wb").write(b"NOTACKPT" + raw[8:])
    with pytest.raises(checkpoint.CheckpointError, match="wrong magic"):
        checkpoint.read_header(p)
    open(p, "wb").write(raw[:8] + struct.pack("<I", 2) + raw[12:])
    with pytest.raises(checkpoint.CheckpointError, match="format version 2"):
        checkpoint.read_header(p)
    rec2, _ = synthetic(info)
    write_synthetic(p, dict(info, version=2), rec2, None)
    with pytest.raises(checkpoint.CheckpointError, match="state version 2"):
        checkpoint.read_header(p)


def test_a_wrong_fingerprint_is_named(good):
    path, info, rec = good
    saved = checkpoint.read_header(path)["info"]
    checkpoint.check_identity(saved, info)
    with pytest.raises(checkpoint.CheckpointError, match="identity mismatch.*topology fingerprint"):
        checkpoint.check_identity(saved, dict(info, topology=info["topology"] ^ 1))
    for k, v in (("nkvecs", 337), ("half_k", 0), ("lj_rcut", 9.0), ("factor", 1.0), ("n_mol", 8)):
        with pytest.raises(checkpoint.CheckpointError, match=f"identity mismatch.*{k}"):
            checkpoint.check_identity(saved, dict(info, **{k: v}))
    checkpoint.check_identity(saved, dict(info, steps_done=0, temps_on=0, R=99))   # mode and scalars are no identity


class _FailingFile:
    """A binary file that raises once more than `limit` bytes have been written to it."""

    def __init__(self, path, limit):
        self.f, self.left = open(path, "wb"), limit

    def write(self, data):
        n = len(data)
        if n > self.left:
            self.f.write(bytes(data[:self.left]))
            self.left = 0
            raise OSError("injected: the disk is full")
        self.left -= n
        return self.f.write(data)

    def __getattr__(self, name):
        return getattr(self.f, name)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.f.close()


def test_a_writer_that_dies_leaves_the_previous_checkpoint(good, tmp_path):
    path, info, rec = good
    before = open(path, "rb").read()
    rec2, _ = synthetic(info, seed=99)
    assert rec2.tobytes() != rec.tobytes()
    for limit in (0, 10, 500, len(before) // 2, len(before) - 1, len(before) + 100):
        # (the last: every part is written, the rewrite of the header fails)
        with pytest.raises(OSError, match="injected"):
            write_synthetic(path, info, rec2, synthetic_extra(10),
                            _open=lambda p, mode, limit=limit: _FailingFile(p, limit))
        assert open(path, "rb").read() == before
        assert not os.path.exists(path + ".tmp")
        assert sorted(os.listdir(tmp_path)) == ["good.ckpt"]

    def dies(r0, n):
        if r0:
            raise KeyboardInterrupt
        return np.ascontiguousarray(rec2[r0:r0 + n])
    with pytest.raises(KeyboardInterrupt):
        checkpoint.write(path, info, info["R"], dies, chunk_records=4)
    assert open(path, "rb").read() == before and not os.path.exists(path + ".tmp")
    write_synthetic(path, info, rec2, None)                              # and a writer that lives replaces it
    assert np.concatenate([c for _, c in checkpoint.iter_chunks(path)]).tobytes() == rec2.tobytes()


@pytest.mark.parametrize("R, n_mol, what", ((10, 9, "n_mol"), (4, 7, "10 replicas")))
def test_load_refuses_another_systems_checkpoint_before_the_library(good, R, n_mol, what):
    path, info, rec = good
    fake = common.fake_batch("load", R=R, n_mol=n_mol)               # _L fails the test when reached
    with pytest.raises(checkpoint.CheckpointError, match=f"identity mismatch.*{what}"):
        fake.load(path)


def test_load_refuses_a_damaged_file_before_the_library(good, tmp_path):
    path, info, rec = good
    raw = bytearray(open(path, "rb").read())
    fake = common.fake_batch("load", R=10, n_mol=7)
    raw[-5] ^= 0xFF
    p = str(tmp_path / "bad.ckpt")
    open(p, "wb").write(raw)
    with pytest.raises(checkpoint.CheckpointError, match="CRC mismatch in record chunk 2"):
        fake.load(p)
    open(p, "wb").write(raw[:-64])
    with pytest.raises(checkpoint.CheckpointError, match="truncated"):
        fake.load(p)


def test_get_and_set_state_check_their_arrays_before_the_library():
    fake = common.fake_batch("set_state get_state", R=4, n_mol=7)
    info = make_info()
    rb = checkpoint.record_layout(info)[1]
    for bad in (np.zeros((2, rb - 64), dtype=np.uint8), np.zeros((2, rb), dtype=np.int8), np.zeros(rb, dtype=np.uint8),
                np.zeros((2, 2 * rb), dtype=np.uint8)[:, ::2], [[0] * rb]):
        with pytest.raises(ValueError, match="records: a C-contiguous uint8 array"):
            fake.set_state(info, bad)
    with pytest.raises(ValueError, match="outside 0..4"):
        fake.set_state(info, np.zeros((3, rb), dtype=np.uint8), r0=2)
    with pytest.raises(ValueError, match="outside 0..4"):
        fake.get_state(r0=3, nr=2)
