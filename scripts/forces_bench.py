#!/usr/bin/env python3
"""Forces and torques (mmc_batch_forces) against deletion energies (mmc_batch_deletion) on one GPU.

750-molecule SPC/E (NIST config 4), R replicas (default 4096 and 61 440), one process per run of
this script.  After a warm-up of every call, --rounds alternating rounds of
  (a) forces(sel=None) with fsum only                 R x 750 wave units
  (b) deletion(sel=None) with esum only               R x 750 wave units, existing code
  (c) forces(sel = 64 molecules) with fsum only       the intended per-block cost
  (d) one sweep: Batch.run of 750 steps, bench.py's default mode
each call synchronous (it returns after the device is done), one call per figure and round.  The
JSON has every round's seconds, the medians and min-max spreads, the ratio (a) / (b) and (a) as a
fraction of a sweep.  A force unit does strictly more than a deletion unit (an exp and a reciprocal
per atom pair, eleven wave sums instead of three): the ratio is recorded, not gated.

    python3 scripts/forces_bench.py [--replicas 4096 61440] [--rounds 7] [--out FILE]
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
MASS = (15.9994, 1.00794, 1.00794)


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
    state = {"e": b.potential_ewald(as_array=True)["energy"].copy(), "seed": 11}
    # a short run first: the replicas leave the common starting point, as in a production block
    state["e"], _ = b.run(64, T, DR, DPHI, seed=10, energies=state["e"], n_groups=2, n_threads=1)
    sel64 = np.random.default_rng(1).choice(n, size=64, replace=False)

    def forces_all():
        b.forces(mass=MASS)

    def deletion_all():
        b.deletion(T)

    def forces_64():
        b.forces(sel=sel64, mass=MASS)

    def sweep():
        state["seed"] += 1
        state["e"], _ = b.run(n, T, DR, DPHI, seed=state["seed"], energies=state["e"], n_groups=2, n_threads=1)

    calls = (("forces_all", forces_all), ("deletion_all", deletion_all), ("forces_sel64", forces_64),
             ("sweep", sweep))
    for _ in range(2):                       # warm-up: first-call allocations, code load
        for _, fn in calls:
            fn()
    t = {name: [] for name, _ in calls}
    for _ in range(rounds):
        for name, fn in calls:
            t[name].append(timed(fn))
    res = b.forces(mass=MASS)
    b.close()
    out = {name: stats(x) for name, x in t.items()}
    a_med, b_med = out["forces_all"]["median"], out["deletion_all"]["median"]
    fs = res["fsum"]
    out.update({
        "replicas": R, "molecules": n, "units_per_call": R * n, "rows_out": False,
        "forces_units_per_s": R * n / a_med, "deletion_units_per_s": R * n / b_med,
        "forces_over_deletion": a_med / b_med,
        "forces_over_sweep": a_med / out["sweep"]["median"],
        "n_summed": float(fs[:, 0].sum()), "n_flagged": int(res["n_flagged"].sum()),
        "mean_f2": float(fs[:, 1].sum() / fs[:, 0].sum()), "mean_tau2": float(fs[:, 2].sum() / fs[:, 0].sum()),
        "max_abs_sum_f": float(np.abs(fs[:, 4:7]).max()),
    })
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, nargs="+", default=[4096, 61440])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    a = mio.load_nist_fixture(4, "unwrapped")
    res = {"bench": "forces", "rounds": args.rounds, "mass": list(MASS),
           "runs": [measure(a, R, args.rounds) for R in args.replicas]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
