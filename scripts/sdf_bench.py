#!/usr/bin/env python3
"""One sdf call (spatial distribution function, mmc_batch_sdf) against one orient_corr call and one
rdf_sites call, on one GPU, one process: 750-molecule SPC/E (NIST config 4) at bench.py's headline
replica count, the shapes of scripts/orient_bench.py.

After a warm-up of all sides, --rounds rounds of
  (a1) one sdf(24, 0.25, fold = 3, site_mask = 1) call, summed output: 27648 cells (108 KB of LDS a
       workgroup), N (N - 1) oxygen deposits per replica, each three dot products and three cells;
  (a7) the same with site_mask = 7: oxygens and hydrogens, three times the deposits;
  (b)  one orient_corr(200, r_max = L / 2) call, summed output: the same walk, four atomics a pair;
  (c)  one rdf_sites(200, r_max = L / 2) call: the six site-site histograms,
taken in turn (a1, a7, b, c, a1, ...) so that drift hits all alike.  Every call is synchronous: it
returns after the device is done and the output is on the host.  The JSON has every sample, medians
and the spread (min, max), the ratios of the medians to (b) and (c), and the fraction of deposits
inside the cube.  The yardsticks are (b) and (c) of the same run; no ratio is a bar.

    python3 scripts/sdf_bench.py [--replicas 61440] [--rounds 7] [--out profiles/sdf_bench.json]
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
NUMBINS = 200
N_HALF, CELL, FOLD = 24, 0.25, 3


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    return {"ms": ms, "median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def one_size(a, R, rounds):
    box = float(a["box"])
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, 5.6 / box,
              structs.factor, RCUT, RCUT)
    b.set_option("device_moves", 1)
    e = b.potential_ewald(as_array=True)["energy"].copy()
    e, _ = b.run(64, T, DR, DPHI, seed=11, energies=e, n_groups=2, n_threads=1)   # replicas diverge

    sides = {"sdf_mask1": lambda: b.sdf(N_HALF, CELL, FOLD, 1),
             "sdf_mask7": lambda: b.sdf(N_HALF, CELL, FOLD, 7),
             "orient_corr": lambda: b.orient_corr(NUMBINS, box / 2),
             "rdf_sites_six_rows": lambda: b.rdf_sites(NUMBINS, box / 2)}
    for _ in range(2):                      # warm-up: code load, first allocations, the LDS opt-in
        out = {k: f() for k, f in sides.items()}
    n = a["com"].shape[0]
    deposits = n * (n - 1) * R
    for k, n_sel in (("sdf_mask1", 1), ("sdf_mask7", 3)):
        s = out[k]
        assert int(s.grid.sum()) + int(s.outside) + int(s.noframe) == deposits * n_sel and int(s.noframe) == 0
    ms = {k: [] for k in sides}
    for _ in range(rounds):
        for k, f in sides.items():
            ms[k].append(timed(f)[0])
    b.close()
    res = {"replicas": R, "n_mol": int(n), "n_half": N_HALF, "cell": CELL, "fold": FOLD,
           "cells": int(out["sdf_mask1"].grid.size), "numbins": NUMBINS, "r_max": box / 2}
    res.update({k: summary(v) for k, v in ms.items()})
    for k, n_sel in (("sdf_mask1", 1), ("sdf_mask7", 3)):
        res[k]["inside_fraction"] = float(out[k].grid.sum() / (deposits * n_sel))
        res[k]["deposits_per_s"] = deposits * n_sel / (res[k]["median_ms"] * 1e-3)
        for y in ("orient_corr", "rdf_sites_six_rows"):
            res[k]["over_" + y] = res[k]["median_ms"] / res[y]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", default="61440")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    a = mio.load_nist_fixture(4, "unwrapped")
    res = {"bench": "sdf", "system": "SPC/E, NIST configuration 4",
           "sizes": [one_size(a, int(r), args.rounds) for r in args.replicas.split(",")]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
