#!/usr/bin/env python3
"""One volume_perturb call (virtual volume moves, mmc_batch_volume_perturb) against the
state-changing composition it replaces, on one GPU, one process: 750-molecule SPC/E (NIST config 4).

Per replica count, after a warm-up of every side, --rounds rounds of
  (a2) one volume_perturb call with K = 2 test boxes (+-dv);
  (b2) on a twin batch with per-replica boxes holding the same states, K = 2 times
       (volume_trial_replicas + volume_settle rejecting all);
  (a8), (b8) the same with K = 8;
  (s)  one sweep of trial moves (n_mol steps of mmc_batch_run), for scale,
taken alternately (a2, b2, a8, b8, s, a2, ...) so that drift hits all alike.  Every call is
synchronous.  The call's scratch is bounded (replicas are processed in chunks), so the replica count
is limited by the two batches' own memory, not by the call; the counts run are recorded.  The JSON has
every sample, medians and the spread, the ratios a / b, and the bar a <= b at both K as "meets_bar",
recorded, not enforced.

    python3 scripts/volume_perturb_bench.py [--replicas 4096,16384] [--rounds 5] [--out profiles/volume_perturb_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import io as mio, observables as obs, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402

T, DR, DPHI, RCUT, ALPHA = 298.15, 0.316555789, 0.05, 10.0, 5.6
DV = 50.0  # A^3: dv / V = 0.2 %


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    return {"ms": ms, "median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def one_size(a, R, rounds):
    box, n = float(a["box"]), a["com"].shape[0]
    V = box ** 3

    def batch():
        b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, ALPHA / box,
                  structs.factor, RCUT, RCUT)
        b.set_option("device_moves", 1)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        e, _ = b.run(64, T, DR, DPHI, seed=11, energies=e, n_groups=2, n_threads=1)   # replicas diverge
        return b, e

    b, e = batch()
    twin, _ = batch()                        # the same seed: the same states
    twin.set_boxes(np.full(R, box), ALPHA)
    twin.recip_long()
    dvs = {2: [DV, -DV], 8: [DV * m for m in (1, -1, 2, -2, 3, -3, 4, -4)]}
    scales = {K: [((V + dv) / V) ** (1.0 / 3.0) for dv in v] for K, v in dvs.items()}
    reject = np.zeros(R, dtype=np.int32)

    def side_a(K):
        return b.volume_perturb(T, scales[K])

    def side_b(K):
        for f in scales[K]:
            tot = twin.volume_trial_replicas(np.full(R, f * box))
            twin.volume_settle(reject)
        return tot

    def sweep():
        nonlocal e
        e, _ = b.run(n, T, DR, DPHI, seed=12, energies=e, n_groups=2, n_threads=1)

    for _ in range(2):                      # warm-up: code load, first allocations
        for K in (2, 8):
            bs, _ = side_a(K)
            side_b(K)
    sweep()
    t = {"a2": [], "b2": [], "a8": [], "b8": [], "sweep": []}
    for _ in range(rounds):
        t["a2"].append(timed(lambda: side_a(2))[0])
        t["b2"].append(timed(lambda: side_b(2))[0])
        t["a8"].append(timed(lambda: side_a(8))[0])
        t["b8"].append(timed(lambda: side_b(8))[0])
        t["sweep"].append(timed(sweep)[0])
    bs, _ = side_a(2)
    p = obs.pressure_from_volume_perturbation(bs, 1, dvs[2], T)
    b.close()
    twin.close()
    res = {"replicas": R, "n_mol": int(n), "dv_A3": DV,
           "volume_perturb_K2": summary(t["a2"]), "trial_settle_x2": summary(t["b2"]),
           "volume_perturb_K8": summary(t["a8"]), "trial_settle_x8": summary(t["b8"]),
           "one_sweep_of_trial_moves": summary(t["sweep"]),
           "two_sided_pooled_pressure_K_per_A3_one_frame": float(p["two_sided_pooled"][0])}
    for K in (2, 8):
        res[f"a_over_b_median_K{K}"] = (res[f"volume_perturb_K{K}"]["median_ms"]
                                        / res[f"trial_settle_x{K}"]["median_ms"])
    res["meets_bar"] = bool(res["a_over_b_median_K2"] <= 1.0 and res["a_over_b_median_K8"] <= 1.0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", default="4096,16384")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    a = mio.load_nist_fixture(4, "unwrapped")
    res = {"bench": "volume_perturb", "system": "SPC/E, NIST configuration 4",
           "sizes": [one_size(a, int(r), args.rounds) for r in args.replicas.split(",")]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
