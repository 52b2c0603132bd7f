#!/usr/bin/env python3
"""What moving a batch's state costs: the bulk record calls beside the per-replica loop they replace,
at bench.py's headline shape (61440 replicas of NIST configuration 4, 750 molecules).

    python scripts/checkpoint_bench.py [--replicas 61440] [--repeats 3] [--out profiles/checkpoint_bench.json]
    python scripts/checkpoint_bench.py --loop-only [--package-root DIR]      # only the get_replica loop

Recorded, not gated.  In one process, on a batch that has run a few steps:
  - get_state and set_state of every replica, with each delivery of the kernels (option
    "state_delivery": 0 = device staging and a copy, 1 = the kernel reads / writes the mapped pinned
    buffer itself), the variants taken in turn, `--repeats` times: seconds, bytes, GB/s;
  - for scale, plain hipMemcpy between a pinned host buffer and device memory of the same byte
    count in pieces of the staging's size (the ceiling the link allows; no kernel, no host copy);
  - the path the bulk calls replace: a loop of get_replica(r), which includes sum_old, over
    `--loop-replicas` replicas;
  - a full Batch.save and Batch.load to a local file.
`--loop-only` prints the loop's JSON alone; with `--package-root` it imports the package from a
checkout of the parent commit (built there), and `--parent-json` merges that output here.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_batch(replicas, steps):
    import bench
    from metropolismontecarlo_amd import io as mio, sharding, structs
    from metropolismontecarlo_amd.device import Batch
    a = mio.load_nist_fixture(4, "unwrapped")
    box = a["box"]
    b = Batch(replicas, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, 5.6 / box,
              structs.factor, bench.RCUT, bench.RCUT)
    b.set_option("device_moves", 1)
    b.set_option("accept_on_device", 1)
    e = b.potential_ewald(as_array=True)["energy"].copy()
    if steps:   # (replicas that differ, S buffers of both parities)
        e, _ = b.run(steps, bench.TEMPERATURE, bench.DR_MAX, bench.DPHI_MAX, sharding.run_seed(phase=0), e, n_groups=2,
                     n_threads=8)
    return b, e


def replica_loop(b, n):
    t0 = time.perf_counter()
    nbytes = 0
    for r in range(n):
        com, coords, s = b.get_replica(r)
        nbytes += com.nbytes + coords.nbytes + s.nbytes
    dt = time.perf_counter() - t0
    return dict(replicas=n, seconds=dt, bytes=nbytes, us_per_replica=1e6 * dt / n, gb_per_s=nbytes / dt / 1e9)


def memcpy_ceiling(total, piece):
    """hipMemcpy of `total` bytes in pieces of `piece` between one pinned buffer and device memory."""
    from metropolismontecarlo_amd import _lib
    hip = C.CDLL(_lib.LIB_PATH)       # the HIP runtime the library itself is linked against
    h, d = C.c_void_p(), C.c_void_p()
    assert hip.hipHostMalloc(C.byref(h), C.c_size_t(piece), 0) == 0
    assert hip.hipMalloc(C.byref(d), C.c_size_t(piece)) == 0
    C.memset(h, 1, piece)
    out = {}
    for name, kind, dst, src in (("device_to_host", 2, h, d), ("host_to_device", 1, d, h)):
        hip.hipMemcpy(dst, src, C.c_size_t(piece), kind)        # (first touch)
        done, t0 = 0, time.perf_counter()
        while done < total:
            n = min(piece, total - done)
            assert hip.hipMemcpy(dst, src, C.c_size_t(n), kind) == 0
            done += n
        dt = time.perf_counter() - t0
        out[name] = dict(seconds=dt, bytes=total, gb_per_s=total / dt / 1e9, piece_bytes=piece)
    hip.hipFree(d)
    hip.hipHostFree(h)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=61440)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loop-replicas", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--parent-json", default=None)
    ap.add_argument("--file-dir", default=None, help="where save() writes (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checkpoint_bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import numpy as np

    if args.loop_only:
        b, _ = make_batch(args.replicas, args.steps)
        replica_loop(b, 64)
        print(json.dumps(replica_loop(b, args.loop_replicas)))
        b.close()
        return

    from metropolismontecarlo_amd import checkpoint
    b, e = make_batch(args.replicas, args.steps)
    info = b.state_info()
    rb = checkpoint.record_layout(info)[1]
    total = args.replicas * rb
    rec = np.empty((args.replicas, rb), dtype=np.uint8)
    rec.fill(1)                                             # (touch every page before anything is timed)
    res = {"get_state": {0: [], 1: []}, "set_state": {0: [], 1: []}}
    b.get_state(0, min(args.replicas, 4096))                # (staging allocated, kernels loaded)
    for _ in range(args.repeats):
        for delivery in (0, 1):
            b.set_option("state_delivery", delivery)
            t0 = time.perf_counter()
            b.get_state(out=rec)
            res["get_state"][delivery].append(time.perf_counter() - t0)
        for delivery in (0, 1):
            b.set_option("state_delivery", delivery)
            t0 = time.perf_counter()
            b.set_state(info, rec)
            res["set_state"][delivery].append(time.perf_counter() - t0)
    b.set_option("state_delivery", -1)                      # (the default: each call's faster one)
    check = b.get_state(0, 64)
    assert check.tobytes() == rec[:64].tobytes()            # set_state put back what get_state took

    def summary(times):
        t = statistics.median(times)
        return dict(seconds_median=t, seconds_min=min(times), seconds_all=times, bytes=total, gb_per_s=total / t / 1e9,
                    us_per_replica=1e6 * t / args.replicas)
    names = {0: "device_staging_then_copy", 1: "mapped_pinned_direct"}
    out = {"shape": dict(replicas=args.replicas, system="NIST SPC/E configuration 4 (750 molecules)",
                         record_bytes=rb, total_bytes=total, steps_before=args.steps, repeats=args.repeats),
           "gated": False}
    for call in ("get_state", "set_state"):
        out[call] = {names[d]: summary(res[call][d]) for d in (0, 1)}
    staging = min(args.replicas, max(1, (64 << 20) // rb)) * rb
    out["pinned_hipMemcpy"] = memcpy_ceiling(total, staging)
    replica_loop(b, 64)
    out["get_replica_loop"] = replica_loop(b, min(args.loop_replicas, args.replicas))
    best_get = min(out["get_state"].values(), key=lambda v: v["seconds_median"])
    out["get_state_vs_loop_per_replica"] = out["get_replica_loop"]["us_per_replica"] / best_get["us_per_replica"]
    if args.parent_json:
        with open(args.parent_json) as fh:
            out["get_replica_loop_parent_commit"] = json.loads(fh.read().strip().splitlines()[-1])
    d = args.file_dir or tempfile.mkdtemp()
    path = os.path.join(d, "checkpoint_bench.ckpt")
    try:
        t0 = time.perf_counter()
        b.save(path, extra=dict(energies=e))
        t_save = time.perf_counter() - t0
        size = os.path.getsize(path)
        t0 = time.perf_counter()
        extra = b.load(path)
        t_load = time.perf_counter() - t0
        assert extra["energies"].tobytes() == e.tobytes()
        assert b.get_state(0, 64).tobytes() == rec[:64].tobytes()
        out["save_load"] = dict(file_bytes=size, save_seconds=t_save, load_seconds=t_load,
                                save_gb_per_s=size / t_save / 1e9, load_gb_per_s=size / t_load / 1e9,
                                note="load reads the file twice: every CRC32 is checked before the batch is touched")
    except OSError as err:
        out["save_load"] = dict(error=str(err))
    finally:
        if os.path.exists(path):
            os.remove(path)
        if not args.file_dir:
            os.rmdir(d)
    b.close()
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: out[k] for k in ("get_state_vs_loop_per_replica",)}))


if __name__ == "__main__":
    main()
