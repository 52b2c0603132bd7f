#!/usr/bin/env python3
"""What the mean force, field and potential on the fixed solute cost at bench.py's headline shape.

    python scripts/solute_force_bench.py [--replicas 61440] [--out profiles/solute_force_bench.json]

61440 replicas of NIST configuration 4 (750 molecules) with a solute in the largest cavity of the
configuration, no moves; bench.py itself is not touched.  In one process, on one batch, the wall time of
  Batch.solute_forces()               force, torque and flags,
  Batch.solute_forces(details=True)   ... and site_lj, field, phi, recip of every site,
  Batch.solute_energy()               the pair energy of every replica,
  Batch.rdf_solute(200, 10.0)         the radial histograms of the same batch,
five calls each after one untimed, taken in turn, for united-atom methane, for a three-site charged solute
(the batch's own molecule as a foreign solute) and for a 16-site one (SPC/E's oxygen row on every site,
charges +-0.1): solute_chain_bench.py's and hydration_map_bench.py's solutes.  Each is also given as a ratio
to the two older observables.  Recorded, not gated.  Writes one JSON object.
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

NUMBINS, R_MAX, TIMED = 200, 10.0, 5


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
    calls = {"forces_ms": lambda: b.solute_forces(),
             "forces_details_ms": lambda: b.solute_forces(details=True),
             "solute_energy_ms": lambda: b.solute_energy(),
             "rdf_solute_ms": lambda: b.rdf_solute(NUMBINS, R_MAX)}
    res = {"shape": {"replicas": args.replicas, "system": "NIST SPC/E configuration 4 (750 molecules)",
                     "rdf_numbins": NUMBINS, "rdf_r_max": R_MAX, "timed_calls": TIMED},
           "gated": False, "results": {}}
    for sol, mol in (solute_for("methane", a), solute_for("charged3", a), (big, np.vstack([c + big.offsets, c]))):
        b.set_solute(sol, mol)
        b.recip_long()
        t = {k: [] for k in calls}
        for k in range(TIMED + 1):
            for name, f in calls.items():
                t0 = time.perf_counter()
                out = f()                       # (every call returns synchronised)
                if k:
                    t[name].append(1e3 * (time.perf_counter() - t0))
                if name == "forces_ms":
                    first = out
        r = {"sites": sol.n_sites, "flagged_replicas": int(np.count_nonzero(first["flags"])),
             "mean_abs_force_K_per_A": float(np.abs(first["force"]).mean()),
             **{k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in t.items()}}
        for num in ("forces_ms", "forces_details_ms"):
            for den in ("solute_energy_ms", "rdf_solute_ms"):
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
