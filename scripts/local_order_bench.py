#!/usr/bin/env python3
"""One local_order call (hydrogen bonds and tetrahedral order of every molecule,
mmc_batch_local_order) against one rdf_sites(200) call (the six site-site histograms,
mmc_batch_rdf_sites), on one GPU, one process: 750-molecule SPC/E (NIST config 4) at R = 4096 and at
bench.py's headline replica count.

Per size, after a warm-up of both sides, --rounds rounds of
  (a) one local_order(400) call, summed output: N (N - 1) O-O distances per replica, the selection
      of four neighbours, about five bond candidates per molecule;
  (b) one rdf_sites(200) call: 9 N (N - 1) / 2 site-site distances per replica,
taken alternately (a, b, a, b, ...) so that drift hits both alike.  Every call is synchronous: it
returns after the device is done and the output is on the host.  The JSON has every sample, medians
and the spread (min, max), <n_HB> and <q> of the frame, and the bar (a) <= (b) as "meets_bar",
recorded, not enforced.

    python3 scripts/local_order_bench.py [--replicas 4096,61440] [--rounds 7] [--out profiles/local_order_bench.json]
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
Q_BINS, NUMBINS = 400, 200


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
        return b.local_order(Q_BINS)

    def side_b():
        return b.rdf_sites(NUMBINS)

    for _ in range(2):                      # warm-up: code load, first allocations
        lo, _ = side_a(), side_b()
    n = a["com"].shape[0]
    assert lo["hb_hist"].sum() == 3 * R * n and lo["q_hist"].sum() == lo["q_sum"][:, 1].sum()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(side_a)[0])
        tb.append(timed(side_b)[0])
    b.close()
    res = {"replicas": R, "n_mol": int(n), "q_bins": Q_BINS, "numbins": NUMBINS,
           "local_order": summary(ta), "rdf_sites_six_rows": summary(tb),
           "hbonds_per_molecule": [float(x) for x in obs.hbonds_per_molecule(lo["hb_hist"])],
           "tetrahedral_mean": float(obs.tetrahedral_mean(lo["q_sum"].sum(0)))}
    res["a_over_b_median"] = res["local_order"]["median_ms"] / res["rdf_sites_six_rows"]["median_ms"]
    res["oo_distances_per_s_a"] = n * (n - 1) * R / (res["local_order"]["median_ms"] * 1e-3)
    res["distances_per_s_b"] = 9 * n * (n - 1) / 2 * R / (res["rdf_sites_six_rows"]["median_ms"] * 1e-3)
    res["meets_bar"] = bool(res["a_over_b_median"] <= 1.0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", default="4096,61440")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    a = mio.load_nist_fixture(4, "unwrapped")
    res = {"bench": "local_order", "system": "SPC/E, NIST configuration 4",
           "sizes": [one_size(a, int(r), args.rounds) for r in args.replicas.split(",")]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
