#!/usr/bin/env python3
"""hbond_rings calls (shortest-path rings of the hydrogen-bond graph, mmc_batch_hbond_rings) against
one one-criterion hbond_network call, on one GPU, one process: 750-molecule SPC/E (NIST config 4) at
bench.py's headline replica count, after 64 moves.

After a warm-up of all sides, --rounds rounds of
  (r3)  hbond_rings with n_max = 3 at (3.5 A, 30 degrees): the bond scan, and a search that looks
        only at the partners of every molecule's partners -- approximately the bond phase alone;
  (r6)  n_max = 6 and
  (r8)  n_max = 8 at the same criterion;
  (r8d) n_max = 8 at the denser criterion (3.6 A, 40 degrees);
  (net) one hbond_network call with the criterion (3.5 A, 30 degrees, 0): the same scan, then the
        clusters,
taken in turn (r3, r6, r8, r8d, net, r3, ...) so that drift hits all alike.  Every call returns the
summed histograms and the per-replica stats, is synchronous, and returns after the device is done
and the output is on the host.  The JSON has every sample, medians and the spread (min, max), each
hbond_rings time as a multiple of the hbond_network call, the ring phase's share of r6, r8 and r8d
(1 - r3 / r.), and the ring counts.  No ratio is a bar.

    python3 scripts/rings_bench.py [--replicas 61440] [--rounds 7] [--out profiles/rings_bench.json]
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

    sides = {"hbond_rings_3": lambda: b.hbond_rings(3.5, 30.0, 3),
             "hbond_rings_6": lambda: b.hbond_rings(3.5, 30.0, 6),
             "hbond_rings_8": lambda: b.hbond_rings(3.5, 30.0, 8),
             "hbond_rings_8_dense": lambda: b.hbond_rings(3.6, 40.0, 8),
             "hbond_network_1": lambda: b.hbond_network(3.5, 30.0, 0)}
    for _ in range(2):                      # warm-up: code load, first allocations
        out = {k: f() for k, f in sides.items()}
    n = a["com"].shape[0]
    r3, r6, r8, r8d = (out[k] for k in ("hbond_rings_3", "hbond_rings_6", "hbond_rings_8", "hbond_rings_8_dense"))
    net = out["hbond_network_1"]
    assert np.array_equal(r8["stats"][:, 0], net["stats"][:, 0, 0]) and np.array_equal(r3["stats"][:, 0], r8["stats"][:, 0])
    assert np.array_equal(r6["ring_hist"][:, :7], r8["ring_hist"][:, :7]) and np.array_equal(r3["ring_hist"][:, :4], r8["ring_hist"][:, :4])
    assert int(r8["stats"][:, 7].sum()) == 0 and int(r8["ring_hist"][0].sum()) == int(r8["stats"][:, 1].sum())
    ms = {k: [] for k in sides}
    for _ in range(rounds):
        for k, f in sides.items():
            ms[k].append(timed(f)[0])
    b.close()
    res = {"replicas": R, "n_mol": int(n), "criterion": [3.5, 30.0], "dense_criterion": [3.6, 40.0]}
    res.update({k: summary(v) for k, v in ms.items()})
    base = res["hbond_network_1"]["median_ms"]
    for k in ("hbond_rings_3", "hbond_rings_6", "hbond_rings_8", "hbond_rings_8_dense"):
        res[k + "_over_network"] = res[k]["median_ms"] / base
    for k in ("hbond_rings_6", "hbond_rings_8"):
        res[k + "_ring_phase_share"] = 1.0 - res["hbond_rings_3"]["median_ms"] / res[k]["median_ms"]
    for k, o in (("hbond_rings_8", r8), ("hbond_rings_8_dense", r8d)):
        res[k + "_counts"] = {"bonds_per_molecule": float(2.0 * o["stats"][:, 0].mean() / n),
                              "rings_per_replica": float(o["stats"][:, 1].mean()),
                              "wrapping_rings_per_replica": float(o["stats"][:, 2].mean()),
                              "flagged_replicas": int(o["stats"][:, 7].sum()),
                              "most_rings_through_one_molecule": int(o["stats"][:, 5].max()),
                              "rings_by_size": [int(x) for x in o["ring_hist"][0]],
                              "homodromic_by_size": [int(x) for x in o["ring_hist"][2]]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", default="61440")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    a = mio.load_nist_fixture(4, "unwrapped")
    res = {"bench": "hbond_rings", "system": "SPC/E, NIST configuration 4",
           "sizes": [one_size(a, int(r), args.rounds) for r in args.replicas.split(",")]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
