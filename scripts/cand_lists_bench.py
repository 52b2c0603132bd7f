#!/usr/bin/env python3
"""Steady state of the candidate lists (csrc/mmc_cand.hpp): one batch of NIST configuration 4 run for
many sweeps with option candidate_lists on and off, alternating, so that lists go stale and are rebuilt
-- which bench.py's 784 steps per replica never reach.

    python scripts/cand_lists_bench.py [--replicas 10240] [--sweeps 30] [--rounds 3] [--out profiles/cand_lists_bench.json]

Writes moves/s of every run, the rebuild count and mean interval in sweeps, the share of steps that
scanned in full, the rebuild kernel's time per replica (a call that finds every replica stale against
the same call that finds none) and the bytes allocated."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metropolismontecarlo_amd import io as mio          # noqa: E402
from metropolismontecarlo_amd import structs            # noqa: E402
from metropolismontecarlo_amd.device import Batch       # noqa: E402

T, DR, DPHI, RCUT = 298.15, 0.316555789, 0.05, 10.0


def one_run(a, R, sweeps, lists, skin):
    n_mol = a["com"].shape[0]
    with Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
               5.6 / a["box"], structs.factor, RCUT, RCUT) as b:
        b.set_option("device_moves", 1)
        b.set_option("candidate_lists", lists)
        if skin is not None:
            b.set_option("cand_skin", skin)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        kw = dict(n_groups=2, n_threads=8)
        e, _ = b.run(120, T, DR, DPHI, 11, e, **kw)                      # warm-up, untimed
        moves = acc = 0
        t0 = time.perf_counter()
        for s in range(sweeps):
            e, st = b.run(n_mol, T, DR, DPHI, 12, e, **kw)
            moves += st["moves"]
            acc += st["trans_accept"] + st["rot_accept"]
        dt = time.perf_counter() - t0
        c = b.cand_stats()
        refresh_us = None
        if lists and c["state"] == 1:
            def call():
                t = time.perf_counter()
                b.run(8, T, DR, DPHI, 13, e, **kw)
                return time.perf_counter() - t
            call()
            fresh = min(call() for _ in range(3))
            stale = []
            for _ in range(3):
                b.set_option("cand_skin", c_skin(b, skin))               # marks every replica stale
                stale.append(call())
            refresh_us = 1e6 * (min(stale) - fresh) / R
        drift = float(np.max(np.abs(e - b.potential_ewald(as_array=True)["energy"]) / np.abs(e)))
    rebuilt = c["refreshes"] - (R if lists and c["state"] == 1 else 0)   # beyond the first build
    return dict(lists=lists, moves_per_s=moves / dt, seconds=dt, acceptance=acc / max(moves, 1), drift=drift,
                cand=c, refresh_us_per_replica=refresh_us,
                scan_share=c["scan_steps"] / max(c["scan_steps"] + c["list_steps"], 1),
                rebuilds_per_replica=rebuilt / R,
                mean_interval_sweeps=(sweeps * R / rebuilt) if rebuilt > 0 else None)


def c_skin(b, skin):
    return 2000 if skin is None else skin


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=10240)
    ap.add_argument("--sweeps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skin", type=int, default=None, help="cand_skin in 1/1000 A (default: the library's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cand_lists_bench.json"))
    args = ap.parse_args()
    a = mio.load_nist_fixture(4, "unwrapped")
    runs = []
    for k in range(args.rounds):
        for lists in (0, 1):
            r = one_run(a, args.replicas, args.sweeps, lists, args.skin)
            r["round"] = k
            runs.append(r)
            print(json.dumps({q: r[q] for q in ("round", "lists", "moves_per_s", "scan_share", "rebuilds_per_replica",
                                                "mean_interval_sweeps", "refresh_us_per_replica")}), flush=True)
    off = [r["moves_per_s"] for r in runs if not r["lists"]]
    on = [r["moves_per_s"] for r in runs if r["lists"]]
    out = dict(replicas=args.replicas, sweeps=args.sweeps, skin_milli=args.skin, runs=runs,
               off_moves_per_s=off, on_moves_per_s=on, ratio_of_means=float(np.mean(on) / np.mean(off)),
               every_on_above_every_off=bool(min(on) > max(off)),
               spread_off=float((max(off) - min(off)) / np.mean(off)), spread_on=float((max(on) - min(on)) / np.mean(on)))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("ratio_of_means", "every_on_above_every_off", "spread_off", "spread_on")}))


if __name__ == "__main__":
    main()
