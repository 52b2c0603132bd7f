#!/usr/bin/env python3
"""What the hydration maps cost at bench.py's headline shape.

    python scripts/hydration_map_bench.py [--replicas 61440] [--out profiles/hydration_map_bench.json]

61440 replicas of NIST configuration 4 (750 molecules) with a charged solute in the largest cavity of the
configuration, no moves; bench.py itself is not touched.  In one process, on one batch, the wall time of
  Batch.hydration_map(12, 0.5)              all eight channels, summed over the replicas,
  Batch.hydration_map(12, 0.5, channels=1)  the oxygen counts alone,
  Batch.rdf_solute(200, 10.0)               the radial histograms of the same batch,
  Batch.solute_energy()                     the pair energy of every replica,
five calls each after one untimed, taken in turn, for a three-site charged solute (the batch's own
molecule as a foreign solute) and for a 16-site one (SPC/E's oxygen row on every site, charges +-0.1):
solute_chain_bench.py's solutes.  Each map is also given as a ratio to the two older observables.
Recorded, not gated.  Writes one JSON object.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N_HALF, CELL, NUMBINS, R_MAX, TIMED = 12, 0.5, 200, 10.0, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=61440)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import bench
    from solute_chain_bench import cavity, solute_for
    from metropolismontecarlo_amd import io as mio
    from metropolismontecarlo_amd import structs
    from metropolismontecarlo_amd.device import Batch
    a = mio.load_nist_fixture(4, "unwrapped")
    box = a["box"]
    b = Batch(args.replicas, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, 5.6 / box,
              structs.factor, bench.RCUT, bench.RCUT)
    c, _ = cavity(a)
    st = np.asarray(a["atype"][:3]) - 1
    off = np.random.default_rng(2).normal(size=(16, 3)) * 0.8
    big = structs.Solute("sites16", off, np.tile([0.1, -0.1], 8), np.tile(np.asarray(a["eps"])[st][:1, st], (16, 1)),
                         np.tile(np.asarray(a["sig"])[st][:1, st], (16, 1)))
    calls = {"map_all_ms": lambda: b.hydration_map(N_HALF, CELL),
             "map_O_ms": lambda: b.hydration_map(N_HALF, CELL, channels=1),
             "rdf_solute_ms": lambda: b.rdf_solute(NUMBINS, R_MAX),
             "solute_energy_ms": lambda: b.solute_energy()}
    res = {"shape": {"replicas": args.replicas, "system": "NIST SPC/E configuration 4 (750 molecules)", "n_half": N_HALF,
                     "cell": CELL, "per_replica": 0, "rdf_numbins": NUMBINS, "rdf_r_max": R_MAX, "timed_calls": TIMED},
           "gated": False, "results": {}}
    for sol, mol in (solute_for("charged3", a), (big, np.vstack([c + big.offsets, c]))):
        b.set_solute(sol, mol)
        b.recip_long()
        t = {k: [] for k in calls}
        for k in range(TIMED + 1):
            for name, f in calls.items():
                t0 = time.perf_counter()
                out = f()                       # (every call returns synchronised)
                if k:
                    t[name].append(1e3 * (time.perf_counter() - t0))
                if name == "map_all_ms":
                    m = out
        cells = (2 * N_HALF) ** 3
        r = {"sites": sol.n_sites, "deposits_inside_per_channel": int(m[0, :cells].sum()),
             "flagged_waters": int(m[6, cells + 1]),
             **{k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in t.items()}}
        for num in ("map_all_ms", "map_O_ms"):
            for den in ("rdf_solute_ms", "solute_energy_ms"):
                r[f"{num[:-3]}_over_{den[:-3]}"] = r[num]["median"] / r[den]["median"]
        res["results"][sol.name] = r
    b.close()
    text = json.dumps(res, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
