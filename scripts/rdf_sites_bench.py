#!/usr/bin/env python3
"""One pass for all six site-site histograms (mmc_batch_rdf_sites) against the three one-site calls
(mmc_batch_rdf on slots 0, 1, 2), on one GPU, one process: 750-molecule SPC/E (NIST config 4) at
R = 4096 and at bench.py's headline replica count.

Per size, after a warm-up of both sides, --rounds rounds of
  (a) one rdf_sites(200) call: six rows, 9 N (N - 1) / 2 distances per replica;
  (b) rdf(0, 200), rdf(1, 200), rdf(2, 200): three of the six rows, a third of the distances,
taken alternately (a, b, a, b, ...) so that drift hits both alike.  Every call is synchronous: it
returns after the device is done and the histogram is on the host.  Also: the wall time of one sweep
(750 steps) of Batch.run in bench.py's default mode on the same batch, the ratio (a) / sweep, and the
time of dipoles().  The JSON has every sample, medians and the spread (min, max); the bar
(a) <= (b) is recorded as "meets_bar", not enforced.

    python3 scripts/rdf_sites_bench.py [--replicas 4096,61440] [--rounds 7] [--out profiles/rdf_sites_bench.json]
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
        return b.rdf_sites(NUMBINS)

    def side_b():
        return [b.rdf(s, NUMBINS) for s in (0, 1, 2)]

    for _ in range(2):                      # warm-up: code load, first allocations
        ha, hb = side_a(), side_b()
    for row, h in zip((0, 3, 5), hb):       # both sides count the same thing
        assert np.array_equal(ha[row], h)
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(side_a)[0])
        tb.append(timed(side_b)[0])
    b.dipoles()
    td = [timed(b.dipoles)[0] for _ in range(rounds)]
    ts = []
    for k in range(3):
        ms, (e, st) = timed(lambda: b.run(750, T, DR, DPHI, seed=12 + k, energies=e, n_groups=2, n_threads=1))
        ts.append(ms)
    b.close()
    n = a["com"].shape[0]
    res = {"replicas": R, "n_mol": int(n), "numbins": NUMBINS,
           "rdf_sites_six_rows": summary(ta), "rdf_three_calls": summary(tb),
           "dipoles": summary(td), "sweep_750_steps": summary(ts)}
    res["a_over_b_median"] = res["rdf_sites_six_rows"]["median_ms"] / res["rdf_three_calls"]["median_ms"]
    res["a_over_sweep_median"] = res["rdf_sites_six_rows"]["median_ms"] / res["sweep_750_steps"]["median_ms"]
    res["distances_per_s_a"] = 9 * n * (n - 1) / 2 * R / (res["rdf_sites_six_rows"]["median_ms"] * 1e-3)
    res["distances_per_s_b"] = 3 * n * (n - 1) / 2 * R / (res["rdf_three_calls"]["median_ms"] * 1e-3)
    res["meets_bar"] = bool(res["a_over_b_median"] <= 1.0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", default="4096,61440")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    a = mio.load_nist_fixture(4, "unwrapped")
    res = {"bench": "rdf_sites", "system": "SPC/E, NIST configuration 4",
           "sizes": [one_size(a, int(r), args.rounds) for r in args.replicas.split(",")]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
