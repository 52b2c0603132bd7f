#!/usr/bin/env python3
"""Rate of a laddered run beside a scalar-temperature run of the same build, and the time of one
exchange, at bench.py's headline shape.

    python scripts/tempering_bench.py [--repeats 5] [--out profiles/tempering_bench.json]

61440 chains of NIST configuration 4 (750 molecules) as 5120 ladders of 12 rungs, moves drawn and
decided on the device, calls of 20 steps with bench.py's constants; bench.py itself is not touched.
Each repeat is a fresh child process per variant, the variants taken in turn:
  (a) scalar:  no per-replica temperatures, every call at bench.py's temperature,
  (b) equal:   set_temperatures(bench.py's temperature for every replica): the LADDER forms of the
               move kernel on the scalar run's own chains, bit for bit -- what the forms cost,
  (c) ladder:  set_temperatures(geometric 260 ... 400 K) -- other chains than (a): warmer on
               average, more moves accepted and committed -- and after the timed calls
               `--exchanges` calls of mmc_batch_exchange, each timed.
Recorded, not gated.  Writes one JSON object.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_RUNGS = 12


def one(mode, replicas, calls, steps, warmup_calls, threads, exchanges):
    """One measurement in this process: prints a JSON line."""
    import numpy as np
    import bench
    from metropolismontecarlo_amd import io as mio
    from metropolismontecarlo_amd import moves, sharding, structs
    from metropolismontecarlo_amd.device import Batch
    a = mio.load_nist_fixture(4, "unwrapped")
    box = a["box"]
    b = Batch(replicas, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, 5.6 / box,
              structs.factor, bench.RCUT, bench.RCUT)
    b.set_option("device_moves", 1)
    b.set_option("accept_on_device", 1)      # the kernel decides, as in bench.py's headline
    if mode == "ladder":
        b.set_temperatures(np.tile(moves.geometric_ladder(260.0, 400.0, N_RUNGS), replicas // N_RUNGS))
    elif mode == "equal":
        b.set_temperatures(np.full(replicas, bench.TEMPERATURE))
    energies = b.potential_ewald(as_array=True)["energy"].copy()
    kw = dict(n_groups=2, n_threads=threads)
    T, dr, dphi = bench.TEMPERATURE, bench.DR_MAX, bench.DPHI_MAX
    for _ in range(warmup_calls):
        energies, _ = b.run(steps, T, dr, dphi, sharding.run_seed(phase=0), energies, **kw)
    n_moves = n_dev = n_acc = 0
    t0 = time.perf_counter()
    for _ in range(calls):
        energies, st = b.run(steps, T, dr, dphi, sharding.run_seed(phase=1), energies, **kw)  # (returns synchronised)
        n_moves += st["moves"]
        n_dev += st["device_decisions"]
        n_acc += st["trans_accept"] + st["rot_accept"]
    elapsed = time.perf_counter() - t0
    out = {"mode": mode, "moves_per_s": n_moves / elapsed, "elapsed_s": elapsed, "moves": n_moves,
           "device_decisions": n_dev, "accept_ratio": n_acc / n_moves, "energy_sum": float(energies.sum())}
    if mode == "ladder":
        rung = moves.initial_rungs(replicas, N_RUNGS)
        times, att, acc = [], None, None
        for k in range(exchanges):
            t0 = time.perf_counter()
            att, acc = b.exchange(N_RUNGS, energies, rung, sharding.run_seed(phase=1), k, attempt=att, accept=acc)
            times.append(time.perf_counter() - t0)
        out.update(exchange_ms=[1e3 * t for t in times], exchange_attempts=int(att.sum()),
                   exchange_accepts=int(acc.sum()), temperature_upload_bytes=8 * replicas)
    drift = float(np.max(np.abs(energies - b.potential_ewald(as_array=True)["energy"]) / np.abs(energies)))
    out["energy_drift_rel"] = drift
    b.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", choices=("scalar", "equal", "ladder"))
    ap.add_argument("--replicas", type=int, default=61440)
    ap.add_argument("--calls", type=int, default=20, help="timed calls per measurement")
    ap.add_argument("--steps", type=int, default=20, help="steps per call")
    ap.add_argument("--warmup-calls", type=int, default=4)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--exchanges", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=150, help="seconds per child process")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.replicas % N_RUNGS:
        ap.error(f"--replicas must be whole ladders of {N_RUNGS} rungs")
    if args.one:
        one(args.one, args.replicas, args.calls, args.steps, args.warmup_calls, args.threads, args.exchanges)
        return 0
    res = {"scalar": [], "equal": [], "ladder": []}

    def report():
        def summary(key):
            v = [r["moves_per_s"] for r in res[key]]
            return {"moves_per_s_median": statistics.median(v), "moves_per_s_min": min(v), "moves_per_s_max": max(v),
                    "repeats": res[key]}

        out = {"shape": {"replicas": args.replicas, "ladders": args.replicas // N_RUNGS, "rungs": N_RUNGS,
                         "system": "NIST SPC/E configuration 4 (750 molecules)", "steps_per_call": args.steps,
                         "timed_calls": args.calls, "warmup_calls": args.warmup_calls, "host_threads": args.threads,
                         "groups": 2, "device_moves": 1, "accept_on_device": 1,
                         "decided_in_kernel": all(r["device_decisions"] == r["moves"] for v in res.values() for r in v)},
               "gated": False,
               "results": {k: summary(k) for k in res if res[k]}}
        if all(res.values()):
            s, q, l = out["results"]["scalar"], out["results"]["equal"], out["results"]["ladder"]
            out["equal_to_scalar"] = q["moves_per_s_median"] / s["moves_per_s_median"]
            out["ladder_to_scalar"] = l["moves_per_s_median"] / s["moves_per_s_median"]
            # (b) must have run (a)'s chains: the same energies to the last bit
            out["equal_ran_the_scalar_chains"] = all(x["energy_sum"] == y["energy_sum"] and x["accept_ratio"] == y["accept_ratio"]
                                                     for x, y in zip(res["scalar"], res["equal"]))
            out["spread_of_scalar_rel"] = (s["moves_per_s_max"] - s["moves_per_s_min"]) / s["moves_per_s_median"]
            # the first exchange of a process allocates nothing new (set_temperatures did); all are listed
            ex = [t for r in res["ladder"] for t in r["exchange_ms"]]
            out["exchange_ms_median"], out["exchange_ms_min"], out["exchange_ms_max"] = \
                statistics.median(ex), min(ex), max(ex)
        text = json.dumps(out, indent=1)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return out

    for rep in range(args.repeats):
        for mode in ("scalar", "equal", "ladder"):     # in turn within a repeat: drift of the machine hits all alike
            cmd = [sys.executable, os.path.abspath(__file__), "--one", mode, "--replicas", str(args.replicas),
                   "--calls", str(args.calls), "--steps", str(args.steps), "--warmup-calls", str(args.warmup_calls),
                   "--threads", str(args.threads), "--exchanges", str(args.exchanges)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            if p.returncode != 0:        # nothing more is started on the GPU after a failure
                sys.stderr.write(p.stdout + p.stderr)
                print(f"{mode} repeat {rep}: exit status {p.returncode}; stopping", file=sys.stderr)
                return 1
            r = json.loads(p.stdout.strip().splitlines()[-1])
            res[mode].append(r)
            print(f"{mode} #{rep}: {r['moves_per_s']:.4g} moves/s"
                  + (f", exchange {statistics.median(r['exchange_ms']):.2f} ms" if mode == "ladder" else ""), flush=True)
        out = report()               # after every repeat: a session cut short keeps its full repeats
    print(json.dumps({k: out[k] for k in ("equal_to_scalar", "ladder_to_scalar", "spread_of_scalar_rel",
                                          "equal_ran_the_scalar_chains", "exchange_ms_median")}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
