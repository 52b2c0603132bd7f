#!/usr/bin/env python3
"""Deletion energies (mmc_batch_deletion) against Widom insertion (mmc_batch_widom) on one GPU.

750-molecule SPC/E (NIST config 4), R replicas (default 4096 and 61 440), one process per run of
this script.  After a warm-up of every call, --rounds alternating rounds of
  (a) deletion(sel=None) with the histogram and esum only        R x 750 wave units
  (b) widom(n_insert = 750) without outputs                      R x 750 wave units
  (c) deletion(sel = 64 molecules) with the histogram and esum   the intended per-block cost
  (d) one sweep: Batch.run of 750 steps, bench.py's default mode
each call synchronous (it returns after the device is done), one call per figure and round.  The
JSON has every round's seconds, the medians and min-max spreads, and the comparison the design
states: median(a) <= median(b) + (max(b) - min(b)).

    python3 scripts/deletion_bench.py [--replicas 4096 61440] [--rounds 7] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import io as mio, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402

T, DR, DPHI, RCUT = 298.15, 0.316555789, 0.05, 10.0
BINS = (200, -45000.0, -5000.0)


def make(a, R):
    box = float(a["box"])
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, 5.6 / box,
              structs.factor, RCUT, RCUT)
    b.set_option("device_moves", 1)
    return b


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def stats(x):
    return {"seconds": x, "median": float(np.median(x)), "min": float(min(x)), "max": float(max(x))}


def measure(a, R, rounds):
    n = a["com"].shape[0]
    b = make(a, R)
    state = {"e": b.potential_ewald(as_array=True)["energy"].copy(), "draw": 0, "seed": 11}
    # a short run first: the replicas leave the common starting point, as in a production block
    state["e"], _ = b.run(64, T, DR, DPHI, seed=10, energies=state["e"], n_groups=2, n_threads=1)
    bs, no = np.zeros(R), np.zeros(R, dtype=np.int64)
    sel64 = np.random.default_rng(1).choice(n, size=64, replace=False)

    def deletion_all():
        b.deletion(T, bins=BINS)

    def widom_n():
        b.widom(n, T, seed=5, draw0=state["draw"], boltz_sum=bs, n_overlap=no)
        state["draw"] += n

    def deletion_64():
        b.deletion(T, sel=sel64, bins=BINS)

    def sweep():
        state["seed"] += 1
        state["e"], _ = b.run(n, T, DR, DPHI, seed=state["seed"], energies=state["e"], n_groups=2, n_threads=1)

    calls = (("deletion_all", deletion_all), ("widom_n", widom_n), ("deletion_sel64", deletion_64),
             ("sweep", sweep))
    for _ in range(2):                       # warm-up: first-call allocations, code load
        for _, fn in calls:
            fn()
    t = {name: [] for name, _ in calls}
    for _ in range(rounds):
        for name, fn in calls:
            t[name].append(timed(fn))
    res = b.deletion(T, bins=BINS)
    b.close()
    out = {name: stats(x) for name, x in t.items()}
    a_med, b_st = out["deletion_all"]["median"], out["widom_n"]
    out.update({
        "replicas": R, "molecules": n, "units_per_call": R * n, "du_out": False,
        "deletion_units_per_s": R * n / a_med, "widom_units_per_s": R * n / b_st["median"],
        "deletion_over_widom": a_med / b_st["median"],
        "deletion_over_sweep": a_med / out["sweep"]["median"],
        "bar": {"median_a": a_med, "median_b": b_st["median"], "spread_b": b_st["max"] - b_st["min"],
                "met": bool(a_med <= b_st["median"] + (b_st["max"] - b_st["min"]))},
        "hist_inside": int(res["hist"][1:-1].sum()), "hist_total": int(res["hist"].sum()),
        "n_flagged": int(res["n_flagged"].sum()),
    })
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, nargs="+", default=[4096, 61440])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    a = mio.load_nist_fixture(4, "unwrapped")
    res = {"bench": "deletion", "rounds": args.rounds, "bins": list(BINS),
           "runs": [measure(a, R, args.rounds) for R in args.replicas]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
