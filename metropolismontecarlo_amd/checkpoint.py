"""The checkpoint file of a replica batch (Batch.save / Batch.load) and what can be done with it
without any device: read_header, read_replica, verify, and record_layout, the pure-Python mirror of
mmc_state_record_layout (include/mmc_hip.h, "Save and resume").

One file, three parts:
  1. 8 bytes magic b"MMCCKPT1", uint32 format version, uint64 length of part 2 (little endian);
  2. a JSON header: the fields of mmc_state_info, `replica0` (global index of the file's first
     replica: a rank saves its own shard), the record layout, the directory of `extra` (dtype, shape,
     offset, CRC32 of each array) and a CRC32 (zlib) per chunk of records;
  3. the raw bytes of the `extra` arrays, then the records, each part starting on 64 bytes.
The file is written to path + ".tmp", flushed and fsynced, then os.replace'd over `path`: a writer
that dies leaves the previous checkpoint intact.  Writer and readers hold one chunk in memory.
"""
import ctypes as C
import json
import os
import struct
import zlib

import numpy as np

from ._lib import StateInfo

MAGIC = b"MMCCKPT1"
VERSION = 1
_PREFIX = struct.Struct("<8sIQ")
CHUNK_BYTES = 64 << 20      # records per chunk of the file: as many as fit this
STATE_MAGIC = 0x31544154534D434D
STATE_VERSION = 1

IDENTITY = ("magic", "version", "n_mol", "nkvecs", "half_k", "lj_rcut", "qq_rcut", "topology", "nk", "k_sq_max",
            "factor")   # (R is the file's own: a shard may be loaded into a batch only of its size, Batch.load checks)
_INFO_FIELDS = [n for n, _ in StateInfo._fields_ if n != "reserved"]
_SOLUTE_FIELDS = ("solute_on", "solute_hash")   # both 0 without a solute, and then not in the dict: the
#                                                 header of a file written before there were solutes has neither


class CheckpointError(ValueError):
    """The file is not a checkpoint this package can use: the message names what is wrong."""


def info_to_dict(info):
    """mmc_state_info (a _lib.StateInfo or already a dict) as a dict of ints, floats and the list db."""
    if isinstance(info, dict):
        return dict(info)
    return {n: (list(info.db) if n == "db" else getattr(info, n)) for n in _INFO_FIELDS
            if n not in _SOLUTE_FIELDS or info.solute_on}


def info_from_dict(d):
    info = StateInfo()
    for n in _INFO_FIELDS:
        if n == "db":
            info.db[:] = [float(x) for x in d["db"]]
        elif n not in _SOLUTE_FIELDS or n in d:
            setattr(info, n, d[n])
    return info


def record_layout(info):
    """(offsets[8], record_bytes) of one replica's record: box, temperature, flags, com, coords, S,
    quat, end of the data.  Sections start on 16 bytes, the record is a multiple of 64 bytes."""
    d = info_to_dict(info)
    n_mol, nkvecs, quat = int(d["n_mol"]), int(d["nkvecs"]), int(d["quat_mode"]) != 0
    if not (1 <= n_mol < 1 << 27 and 1 <= nkvecs <= 352):
        raise CheckpointError(f"n_mol {n_mol} or nkvecs {nkvecs} out of range")

    def up(x, a):
        return (x + a - 1) // a * a
    off = [0, 8, 16, 32]
    off.append(up(off[3] + 24 * n_mol, 16))
    off.append(up(off[4] + 72 * n_mol, 16))
    off.append(up(off[5] + 16 * nkvecs, 16))
    off.append(off[6] + (32 * n_mol if quat else 0))
    return off, up(off[7], 64)


def split_record(info, rec):
    """dict(box, temperature, flags, com, coords, S, quat) of one record (uint8 [record_bytes])."""
    d = info_to_dict(info)
    off, nbytes = record_layout(d)
    rec = np.ascontiguousarray(rec, dtype=np.uint8).ravel()
    if rec.shape[0] != nbytes:
        raise CheckpointError(f"a record of this state has {nbytes} bytes, not {rec.shape[0]}")
    n_mol, nk = int(d["n_mol"]), int(d["nkvecs"])

    def f64(o, n):
        return rec[o:o + 8 * n].view(np.float64).copy()
    return dict(box=float(f64(off[0], 1)[0]), temperature=float(f64(off[1], 1)[0]),
                flags=int(rec[off[2]:off[2] + 8].view(np.uint64)[0]),
                com=f64(off[3], 3 * n_mol).reshape(n_mol, 3), coords=f64(off[4], 9 * n_mol).reshape(3 * n_mol, 3),
                S=f64(off[5], 2 * nk).view(np.complex128),
                quat=f64(off[6], 4 * n_mol).reshape(n_mol, 4) if int(d["quat_mode"]) else None)


def _dtype_to_json(dt):
    return [list(x) for x in dt.descr] if dt.names else dt.str


def _dtype_from_json(j):
    return np.dtype([tuple(x) for x in j]) if isinstance(j, list) else np.dtype(j)


def _up64(x):
    return (x + 63) // 64 * 64


def write(path, info, n_records, chunks, extra=None, replica0=0, chunk_records=0, _open=open):
    """Write a checkpoint of n_records records: chunks(r0, n) returns records [r0, r0 + n) as a uint8
    array [n, record_bytes] (Batch.get_state), called once per chunk in order.  `extra`: a dict of
    numpy arrays (structured dtypes included).  Atomic: see the module's text."""
    d = info_to_dict(info)
    off, rb = record_layout(d)
    n_records = int(n_records)
    per = int(chunk_records) if chunk_records else max(1, CHUNK_BYTES // rb)
    n_chunks = (n_records + per - 1) // per
    arrays = {k: np.asarray(v, order="C") for k, v in (extra or {}).items()}   # (a 0-d array stays one)
    directory, pos = {}, 0
    for k, a in arrays.items():
        directory[k] = dict(dtype=_dtype_to_json(a.dtype), shape=list(a.shape), offset=pos, nbytes=int(a.nbytes),
                            crc32=zlib.crc32(a.tobytes()))
        pos = _up64(pos + a.nbytes)
    head = dict(format="metropolismontecarlo_amd checkpoint", version=VERSION, info=d, replica0=int(replica0),
                n_records=n_records, record_bytes=rb, offsets=off, chunk_records=per, extra=directory,
                extra_bytes=pos, chunk_crc32=[0xFFFFFFFF] * n_chunks)

    def encode(h, size=None):
        raw = json.dumps(h).encode("utf-8")
        return raw if size is None else raw + b" " * (size - len(raw))
    head_len = _up64(_PREFIX.size + len(encode(head))) - _PREFIX.size   # (CRCs have at most these ten digits)
    head["data_offset"] = _PREFIX.size + head_len
    head["file_bytes"] = head["data_offset"] + pos + n_records * rb
    head_len = _up64(_PREFIX.size + len(encode(head)) + 64) - _PREFIX.size
    head["data_offset"] = _PREFIX.size + head_len
    head["file_bytes"] = head["data_offset"] + pos + n_records * rb
    tmp = path + ".tmp"
    try:
        with _open(tmp, "wb") as f:
            f.write(_PREFIX.pack(MAGIC, VERSION, head_len))
            f.write(encode(head, head_len))
            for k, a in arrays.items():
                raw = a.tobytes()
                f.write(raw + b"\0" * (_up64(len(raw)) - len(raw)))
            crcs = []
            for c in range(n_chunks):
                r0, n = c * per, min(per, n_records - c * per)
                rec = chunks(r0, n)
                if not (isinstance(rec, np.ndarray) and rec.dtype == np.uint8 and rec.shape == (n, rb)
                        and rec.flags.c_contiguous):
                    raise ValueError(f"chunks({r0}, {n}) must return a C-contiguous uint8 array of shape {(n, rb)}")
                raw = memoryview(rec).cast("B")
                crcs.append(zlib.crc32(raw))
                f.write(raw)
            head["chunk_crc32"] = crcs
            f.seek(_PREFIX.size)
            f.write(encode(head, head_len))
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except FileNotFoundError:
            pass
        raise


def read_header(path):
    """The JSON header as a dict (header["info"] holds the mmc_state_info fields).  Raises
    CheckpointError for a wrong magic or version, a header that does not parse, a truncated file."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        raw = f.read(_PREFIX.size)
        if len(raw) < _PREFIX.size:
            raise CheckpointError(f"{path}: truncated: {len(raw)} bytes, not even the {_PREFIX.size} of the prefix")
        magic, version, head_len = _PREFIX.unpack(raw)
        if magic != MAGIC:
            raise CheckpointError(f"{path}: wrong magic {magic!r}, a checkpoint starts with {MAGIC!r}")
        if version != VERSION:
            raise CheckpointError(f"{path}: format version {version}, this package reads version {VERSION}")
        if _PREFIX.size + head_len > size:
            raise CheckpointError(f"{path}: truncated: the header alone needs {_PREFIX.size + head_len} bytes, the file "
                                  f"has {size}")
        try:
            head = json.loads(f.read(head_len).decode("utf-8"))
        except ValueError as e:
            raise CheckpointError(f"{path}: the header does not parse: {e}") from None
    info = head["info"]
    if info["magic"] != STATE_MAGIC or info["version"] != STATE_VERSION:
        raise CheckpointError(f"{path}: state version {info['version']} (magic {info['magic']:#x}), this package "
                              f"reads state version {STATE_VERSION}")
    off, rb = record_layout(info)
    if off != head["offsets"] or rb != head["record_bytes"]:
        raise CheckpointError(f"{path}: the header's record layout is not that of its own state info")
    if head["file_bytes"] != head["data_offset"] + head["extra_bytes"] + head["n_records"] * rb:
        raise CheckpointError(f"{path}: the header's sizes do not add up")
    if size < head["file_bytes"]:
        raise CheckpointError(f"{path}: truncated: {size} bytes of {head['file_bytes']}")
    if size > head["file_bytes"]:
        raise CheckpointError(f"{path}: {size - head['file_bytes']} bytes beyond the end the header gives")
    return head


def read_extra(path, head=None):
    """The `extra` arrays of the file, each checked against its CRC32."""
    head = read_header(path) if head is None else head
    out = {}
    with open(path, "rb") as f:
        for k, e in head["extra"].items():
            f.seek(head["data_offset"] + e["offset"])
            raw = f.read(e["nbytes"])
            if len(raw) != e["nbytes"] or zlib.crc32(raw) != e["crc32"]:
                raise CheckpointError(f"{path}: CRC mismatch in extra array {k!r}")
            out[k] = np.frombuffer(raw, dtype=_dtype_from_json(e["dtype"])).reshape(e["shape"]).copy()
    return out


def iter_chunks(path, head=None):
    """(r0, records uint8 [n, record_bytes]) of every chunk in order, each checked against its CRC32."""
    head = read_header(path) if head is None else head
    rb, per, n_rec = head["record_bytes"], head["chunk_records"], head["n_records"]
    with open(path, "rb") as f:
        f.seek(head["data_offset"] + head["extra_bytes"])
        for c, crc in enumerate(head["chunk_crc32"]):
            r0, n = c * per, min(per, n_rec - c * per)
            rec = np.fromfile(f, dtype=np.uint8, count=n * rb)
            if rec.shape[0] != n * rb:
                raise CheckpointError(f"{path}: truncated in record chunk {c}")
            if zlib.crc32(memoryview(rec)) != crc:
                raise CheckpointError(f"{path}: CRC mismatch in record chunk {c} (records {r0}..{r0 + n - 1})")
            yield r0, rec.reshape(n, rb)


def verify(path, head=None):
    """Read the whole file once and check every CRC32.  Returns (boxes, temperatures) of the records."""
    head = read_header(path) if head is None else head
    read_extra(path, head)
    off = head["offsets"]
    boxes, temps = np.empty(head["n_records"]), np.empty(head["n_records"])
    for r0, rec in iter_chunks(path, head):
        boxes[r0:r0 + rec.shape[0]] = rec[:, off[0]:off[0] + 8].copy().view(np.float64)[:, 0]
        temps[r0:r0 + rec.shape[0]] = rec[:, off[1]:off[1] + 8].copy().view(np.float64)[:, 0]
    return boxes, temps


def read_replica(path, r, head=None):
    """dict(com, coords, S, box, temperature, quat, flags) of record r of the file (replica
    header["replica0"] + r of the ensemble): a seek to its chunk, which is checked against its CRC32.
    S is in device order (mmc_get_kvectors of a batch with the header's half_k)."""
    head = read_header(path) if head is None else head
    r = int(r)
    if not 0 <= r < head["n_records"]:
        raise IndexError(f"record {r} outside 0..{head['n_records'] - 1}")
    rb, per, n_rec = head["record_bytes"], head["chunk_records"], head["n_records"]
    c = r // per
    r0, n = c * per, min(per, n_rec - c * per)
    with open(path, "rb") as f:
        f.seek(head["data_offset"] + head["extra_bytes"] + r0 * rb)
        rec = np.fromfile(f, dtype=np.uint8, count=n * rb)
    if rec.shape[0] != n * rb:
        raise CheckpointError(f"{path}: truncated in record chunk {c}")
    if zlib.crc32(memoryview(rec)) != head["chunk_crc32"][c]:
        raise CheckpointError(f"{path}: CRC mismatch in record chunk {c} (records {r0}..{r0 + n - 1})")
    return split_record(head["info"], rec[(r - r0) * rb:(r - r0 + 1) * rb])


def check_identity(saved, mine, what="the batch"):
    """Raise CheckpointError naming the first identity field in which two state infos differ."""
    a, b = info_to_dict(saved), info_to_dict(mine)
    for k in IDENTITY:
        if a[k] != b[k]:
            shown = (f"{a[k]:#018x}", f"{b[k]:#018x}") if k == "topology" else (a[k], b[k])
            name = "topology fingerprint" if k == "topology" else k
            raise CheckpointError(f"identity mismatch: the checkpoint's {name} is {shown[0]}, {what} has {shown[1]}")


def library_layout(info):
    """mmc_state_record_layout through the library (a pure host function: no GPU needed)."""
    from . import _lib
    offs, rb = (C.c_int64 * 8)(), C.c_int64()
    sinfo = info if isinstance(info, StateInfo) else info_from_dict(info)
    _lib.check(_lib.lib().mmc_state_record_layout(C.byref(sinfo), offs, C.byref(rb)))
    return list(offs), rb.value
