#!/usr/bin/env python3
"""One cavity call (occupancy statistics of probe spheres, mmc_batch_cavity) against one widom call
(test-particle insertions, mmc_batch_widom) with as many insertions as probes, on one GPU, one
process: 750-molecule SPC/E (NIST config 4) at R = 4096 and at bench.py's headline replica count.

Per size, after a warm-up of both sides, --rounds rounds of
  (a) one cavity(750 probes, 8 radii 0.5 .. 4.0 A, 400 nearest-site bins) call, summed output:
      750 x 750 probe-oxygen distances per replica, eight compares where a wave has a site in range;
  (b) one widom(750 insertions) call: the same 750 points as centres of mass, each with the pair
      energies of its neighbours and the reciprocal sum over the k vectors,
taken alternately (a, b, a, b, ...) so that drift hits both alike.  Every call is synchronous: it
returns after the device is done and the output is on the host.  The JSON has every sample, medians
and the spread (min, max), p_0 at the eight radii, and the bar (a) <= (b) as "meets_bar", recorded,
not enforced.

    python3 scripts/cavity_bench.py [--replicas 4096,61440] [--rounds 7] [--out profiles/cavity_bench.json]
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

T, DR, DPHI, RCUT = 298.15, 0.316555789, 0.05, 10.0
N_PROBE, NN_BINS, NN_MAX, N_CAP = 750, 400, 5.0, 32
RADII = [m * (NN_MAX / NN_BINS) for m in range(40, 321, 40)]      # 0.5 .. 4.0 A, edges of the nearest-site grid


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

    def side_a():
        return b.cavity(N_PROBE, seed=5, radii=RADII, n_cap=N_CAP, nn_bins=NN_BINS, nn_max=NN_MAX)

    def side_b():
        return b.widom(N_PROBE, T, seed=5)

    for _ in range(2):                      # warm-up: code load, first allocations
        cv, _ = side_a(), side_b()
    n = a["com"].shape[0]
    assert np.all(cv["occ_hist"].sum(1) == R * N_PROBE) and cv["nn_hist"].sum() == R * N_PROBE
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(side_a)[0])
        tb.append(timed(side_b)[0])
    b.close()
    _, p0 = obs.cavity_size_distribution(cv["nn_hist"], NN_MAX)
    res = {"replicas": R, "n_mol": int(n), "n_probe": N_PROBE, "radii": RADII, "nn_bins": NN_BINS, "nn_max": NN_MAX,
           "cavity": summary(ta), "widom": summary(tb),
           "p0_at_radii": [float(x) for x in cv["occ_hist"][:, 0] / float(R * N_PROBE)],
           "largest_empty_radius_seen": float(np.flatnonzero(cv["nn_hist"])[-1] * (NN_MAX / NN_BINS)),
           "p0_3p3": float(p0[264])}
    res["a_over_b_median"] = res["cavity"]["median_ms"] / res["widom"]["median_ms"]
    res["probes_per_s_a"] = N_PROBE * R / (res["cavity"]["median_ms"] * 1e-3)
    res["distances_per_s_a"] = N_PROBE * n * R / (res["cavity"]["median_ms"] * 1e-3)
    res["insertions_per_s_b"] = N_PROBE * R / (res["widom"]["median_ms"] * 1e-3)
    res["meets_bar"] = bool(res["a_over_b_median"] <= 1.0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", default="4096,61440")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    a = mio.load_nist_fixture(4, "unwrapped")
    res = {"bench": "cavity", "system": "SPC/E, NIST configuration 4",
           "sizes": [one_size(a, int(r), args.rounds) for r in args.replicas.split(",")]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
