#!/usr/bin/env python3
"""One orient_corr call (orientational pair correlations, mmc_batch_orient_corr) against one
rdf_sites call (the six site-site histograms, mmc_batch_rdf_sites), on one GPU, one process:
750-molecule SPC/E (NIST config 4) at R = 4096 and at bench.py's headline replica count, the shapes
of scripts/rdf_sites_bench.py.

Per size, after a warm-up of both sides, --rounds rounds of
  (a) one orient_corr(200, r_max = L / 2) call, summed output: N (N - 1) / 2 site-0 distances per
      replica, four 64-bit rows; about half of the pairs (those within L / 2) also take three dot
      products, a reciprocal and two more LDS atomics;
  (b) one rdf_sites(200, r_max = L / 2) call: 9 N (N - 1) / 2 site-site distances per replica, six
      32-bit rows,
taken alternately (a, b, a, b, ...) so that drift hits both alike.  Every call is synchronous: it
returns after the device is done and the output is on the host.  The JSON has every sample, medians
and the spread (min, max), the ratio of the medians, the fraction of pairs within L / 2 and the
whole-box Kirkwood factor of the frame.  The yardstick is (b) of the same run; no ratio is a bar.

    python3 scripts/orient_bench.py [--replicas 4096,61440] [--rounds 7] [--out profiles/orient_bench.json]
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
NUMBINS = 200


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
        return b.orient_corr(NUMBINS, box / 2)

    def side_b():
        return b.rdf_sites(NUMBINS, box / 2)

    for _ in range(2):                      # warm-up: code load, first allocations
        oc, six = side_a(), side_b()
    n = a["com"].shape[0]
    pairs = n * (n - 1) // 2 * R
    assert oc[0].sum() == pairs and np.array_equal(oc[0, :-1], six[0].astype(np.int64))
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(side_a)[0])
        tb.append(timed(side_b)[0])
    b.close()
    res = {"replicas": R, "n_mol": int(n), "numbins": NUMBINS, "r_max": box / 2,
           "orient_corr": summary(ta), "rdf_sites_six_rows": summary(tb),
           "pairs_in_range_fraction": float(oc[0, :-1].sum() / pairs),
           "kirkwood_gk_whole_box": float(obs.kirkwood_gk(oc, n, R)[-1]),
           "kirkwood_gk_at_r_max": float(obs.kirkwood_gk(oc, n, R)[-2])}
    res["a_over_b_median"] = res["orient_corr"]["median_ms"] / res["rdf_sites_six_rows"]["median_ms"]
    res["pairs_per_s_a"] = pairs / (res["orient_corr"]["median_ms"] * 1e-3)
    res["distances_per_s_b"] = 9 * pairs / (res["rdf_sites_six_rows"]["median_ms"] * 1e-3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", default="4096,61440")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    a = mio.load_nist_fixture(4, "unwrapped")
    res = {"bench": "orient_corr", "system": "SPC/E, NIST configuration 4",
           "sizes": [one_size(a, int(r), args.rounds) for r in args.replicas.split(",")]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
