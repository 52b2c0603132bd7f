#!/usr/bin/env python3
"""Rate of a Wolf-style chain beside the Ewald chain, at bench.py's headline shape.

    python scripts/wolf_bench.py --parent-tree build/parent_tree [--variant NAME=build/NAME.so ...]
                                 [--repeats 7] [--out profiles/wolf_bench.json]

61440 chains of NIST configuration 4, moves drawn and decided on the device, eight steps per launch,
bench.py's constants, warm-up (prewarm + 64 steps) and timed call (600 steps); bench.py itself is
not touched.  Three things are measured, each in a fresh child process per repeat, the variants
taken in turn within every repeat:
  (a) Ewald moves/s of the PARENT commit: --parent-tree is a checkout of it with its library built
      (`git archive <parent> | tar -x -C build/parent_tree`, then its own build); the child imports
      that tree's package and bench.py, not this one's,
  (b) Ewald moves/s of this tree's library,
  (c) Wolf moves/s of this tree's library -- and of every --variant (builds with another
      WV_OCC_WOLF, scripts/build_variant.sh), Wolf style.
The spread of (a) is what its repeats show; nothing is assumed.  Writes one JSON object.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("MMC_BENCH_TREE") or ROOT)   # (the tree a child measures)


def one(style, replicas, steps, warmup, prewarm, threads):
    """One measurement in this process: prints a JSON line."""
    import numpy as np
    import bench
    from metropolismontecarlo_amd import io as mio
    from metropolismontecarlo_amd import sharding, structs
    from metropolismontecarlo_amd.device import Batch
    a = mio.load_nist_fixture(4, "unwrapped")
    box = a["box"]
    b = Batch(replicas, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, 5.6 / box,
              structs.factor, bench.RCUT, bench.RCUT)
    b.set_option("device_moves", 1)
    b.set_option("accept_on_device", 1)      # the kernel decides, as in bench.py's headline
    total = b.potential_ewald
    if style == "wolf":
        b.recip_long()
        b.set_coulomb_style("wolf")
        total = b.potential_wolf
    energies = total(as_array=True)["energy"].copy()
    kw = dict(n_groups=2, time_kernels=8, n_threads=threads)
    T, dr, dphi = bench.TEMPERATURE, bench.DR_MAX, bench.DPHI_MAX
    if prewarm > 0:
        energies, _ = b.run(prewarm, T, dr, dphi, sharding.run_seed(phase=2), energies, **kw)
    energies, _ = b.run(warmup, T, dr, dphi, sharding.run_seed(phase=0), energies, **kw)
    t0 = time.perf_counter()
    energies, st = b.run(steps, T, dr, dphi, sharding.run_seed(phase=1), energies, **kw)  # (returns synchronised)
    elapsed = time.perf_counter() - t0
    drift = float(np.max(np.abs(energies - total(as_array=True)["energy"]) / np.abs(energies)))
    b.close()
    print(json.dumps({"style": style, "moves_per_s": st["moves"] / elapsed, "elapsed_s": elapsed,
                      "moves": st["moves"], "launches": st["launches"],
                      "kernel_ms_per_launch": st["kernel_ms"] / max(st["timed_launches"], 1),
                      "timed_launches": st["timed_launches"], "device_decisions": st["device_decisions"],
                      "steps_per_launch": st["moves"] / max(st["launches"], 1) / (replicas / 2),   # (two groups)
                      "accept_ratio": (st["trans_accept"] + st["rot_accept"]) / st["moves"],
                      "energy_drift_rel": drift,
                      "tree": "parent" if os.environ.get("MMC_BENCH_TREE") else "this"}))   # (whose package and bench.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", choices=("ewald", "wolf"))
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its library built")
    ap.add_argument("--variant", action="append", default=[], help="NAME=path of another build (Wolf style)")
    ap.add_argument("--replicas", type=int, default=61440)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--prewarm", type=int, default=56)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=150, help="seconds per child process")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.one:
        one(args.one, args.replicas, args.steps, args.warmup, args.prewarm, args.threads)
        return 0
    ptree = os.path.abspath(args.parent_tree or "")
    if not os.path.exists(os.path.join(ptree, "metropolismontecarlo_amd", "libmmc_hip.so")):
        ap.error("--parent-tree: a checkout of the parent commit with its libmmc_hip.so built is required")
    here = os.path.join(ROOT, "metropolismontecarlo_amd", "libmmc_hip.so")
    runs = [("a_parent_ewald", None, "ewald"), ("b_ewald", here, "ewald"), ("c_wolf", here, "wolf")]
    for v in args.variant:
        name, path = v.split("=", 1)
        runs.append((f"c_wolf_{name}", path, "wolf"))
    res = {k: [] for k, _, _ in runs}
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import codeobj_diff

    def report():
        """The JSON object of what has been measured so far; written to --out."""
        def summary(key):
            v = [r["moves_per_s"] for r in res[key]]
            k = [r["kernel_ms_per_launch"] for r in res[key]]
            return {"moves_per_s_median": statistics.median(v), "moves_per_s_min": min(v), "moves_per_s_max": max(v),
                    "kernel_us_per_launch_median": 1e3 * statistics.median(k), "repeats": res[key]}

        out = {"shape": {"replicas": args.replicas, "system": "NIST SPC/E configuration 4 (750 molecules)",
                         "steps": args.steps, "warmup": args.warmup, "prewarm": args.prewarm, "host_threads": args.threads,
                         "groups": 2, "device_moves": 1, "accept_on_device": 1,
                         # what the timed calls recorded, not what was asked for
                         "steps_per_launch": sorted({r["steps_per_launch"] for v in res.values() for r in v}),
                         "decided_in_kernel": all(r["device_decisions"] == r["moves"] for v in res.values() for r in v)},
               "results": {k: summary(k) for k in res}}
        # what the compiler made of the headline's kernel form in every library measured (code-object metadata)
        for key, lib, style in runs:
            lib = lib or os.path.join(ptree, "metropolismontecarlo_amd", "libmmc_hip.so")
            form = "k_move_eval_wave<false, true, true, true>(" if style == "wolf" else "k_move_eval_wave<false, true, true"
            for name, rec in codeobj_diff.kernels(lib).items():
                if form in name and (style == "wolf" or "true, true, true>" not in name):
                    vgpr, lds = rec[".vgpr_count"], rec[".group_segment_fixed_size"]
                    out["results"][key]["kernel"] = {
                        "name": name.split("(")[0], "vgpr_count": vgpr, "scratch_bytes": rec[".private_segment_fixed_size"],
                        "lds_bytes_per_workgroup": lds,
                        # waves per SIMD: 512 VGPRs per lane and SIMD, 160 KB of LDS per CU for workgroups of 4 waves
                        "waves_per_simd_by_registers": min(8, 512 // vgpr), "workgroups_per_cu_by_lds": 163840 // lds}
        a = out["results"]["a_parent_ewald"]
        out["spread_of_a_rel"] = (a["moves_per_s_max"] - a["moves_per_s_min"]) / a["moves_per_s_median"]
        for k in res:
            out["results"][k]["ratio_to_a"] = out["results"][k]["moves_per_s_median"] / a["moves_per_s_median"]
        text = json.dumps(out, indent=1)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return out

    for rep in range(args.repeats):
        for key, lib, style in runs:     # in turn within a repeat: drift of the machine hits all alike
            env = dict(os.environ)
            env.pop("MMC_HIP_LIB", None)
            if lib is None:              # the parent commit: its own package, bench.py and library
                env["MMC_BENCH_TREE"] = ptree
            else:
                env["MMC_HIP_LIB"] = os.path.abspath(lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--one", style, "--replicas", str(args.replicas),
                   "--steps", str(args.steps), "--warmup", str(args.warmup), "--prewarm", str(args.prewarm),
                   "--threads", str(args.threads)]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.timeout)
            if p.returncode != 0:        # nothing more is started on the GPU after a failure
                sys.stderr.write(p.stdout + p.stderr)
                print(f"{key} repeat {rep}: exit status {p.returncode}; stopping", file=sys.stderr)
                return 1
            r = json.loads(p.stdout.strip().splitlines()[-1])
            res[key].append(r)
            print(f"{key} #{rep}: {r['moves_per_s']:.4g} moves/s, {r['kernel_ms_per_launch'] * 1e3:.1f} us/launch",
                  flush=True)
        out = report()               # after every repeat: a session cut short keeps its full repeats
    print(json.dumps({k: {"median": v["moves_per_s_median"], "ratio_to_a": v["ratio_to_a"]}
                      for k, v in out["results"].items()}), f"spread of (a): {out['spread_of_a_rel']:.3%}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
