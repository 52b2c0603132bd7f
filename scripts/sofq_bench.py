#!/usr/bin/env python3
"""One structure_factor call (partial structure factors, mmc_batch_structure_factor) against one
rdf_sites call (the six site-site histograms, mmc_batch_rdf_sites), on one GPU, one process:
750-molecule SPC/E (NIST config 4) at R = 4096 and at bench.py's headline replica count, the shapes
of scripts/rdf_sites_bench.py, at n_max = 8, 16 and 32.

Per size and n_max, after a warm-up of both sides, --rounds rounds of
  (a) one structure_factor(n_max) call, summed output: 3 N phase sums for each of the half-space
      vectors (1054, 8538, 68532) per replica, six 64-bit atomics per vector, the reduce over the
      replicas;
  (b) one rdf_sites(200, r_max = L / 2) call: 9 N (N - 1) / 2 site-site distances per replica,
taken alternately (a, b, a, b, ...) so that drift hits both alike.  Every call is synchronous: it
returns after the device is done and the output is on the host.  The JSON has every sample, medians
and the spread (min, max), the ratio of the medians, atom-vector terms per second and S_OO, S_ZZ of
the lowest shell.  The yardstick is (b) of the same run; no ratio is a bar.

    python3 scripts/sofq_bench.py [--replicas 4096,61440] [--n-max 8,16,32] [--rounds 7] [--out profiles/sofq_bench.json]

--calls K: K structure_factor calls of the first size and first n_max and nothing else timed -- what
a counter run (rocprofv3 --pmc SQ_INSTS_VALU, nothing else traced) wraps.
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
SIMDS, CLOCK_HZ = 1024, 2.4e9          # MI355X: 256 compute units of four SIMDs; a wave instruction takes 4 cycles


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    return {"ms": ms, "median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def make_batch(a, R):
    box = float(a["box"])
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, 5.6 / box,
              structs.factor, RCUT, RCUT)
    b.set_option("device_moves", 1)
    e = b.potential_ewald(as_array=True)["energy"].copy()
    b.run(64, T, DR, DPHI, seed=11, energies=e, n_groups=2, n_threads=1)   # replicas diverge
    return b


def one_size(a, R, n_maxes, rounds):
    box = float(a["box"])
    n = a["com"].shape[0]
    b = make_batch(a, R)
    out = []
    for n_max in n_maxes:
        def side_a():
            return b.structure_factor(n_max)

        def side_b():
            return b.rdf_sites(NUMBINS, box / 2)

        for _ in range(2 if n_max < 32 else 1):      # warm-up: code load, first allocations
            (count, sq), six = side_a(), side_b()
        half = int(count.sum()) // 2
        ta, tb = [], []
        for _ in range(rounds):
            ta.append(timed(side_a)[0])
            tb.append(timed(side_b)[0])
        s, cnt, q = obs.structure_factor_shells(n_max, box)
        part = obs.partial_structure_factors(sq, count, n, ("O", "H", "H"), n_frames=R)
        szz = obs.charge_structure_factor(sq, count, a["charge"][:3], n, n_frames=R)
        res = {"replicas": R, "n_mol": int(n), "n_max": n_max, "half_space_vectors": half,
               "structure_factor": summary(ta), "rdf_sites_six_rows": summary(tb),
               "q_lowest": float(q[0]), "S_OO_lowest": float(part[("O", "O")][0]), "S_ZZ_lowest": float(szz[0]),
               "S_OO_highest": float(part[("O", "O")][-1])}
        res["a_over_b_median"] = res["structure_factor"]["median_ms"] / res["rdf_sites_six_rows"]["median_ms"]
        terms = 3.0 * n * half * R
        res["atom_vector_terms_per_s"] = terms / (res["structure_factor"]["median_ms"] * 1e-3)
        # the vector instructions per atom and half-space vector the chip would issue in that time at
        # its peak of one wave instruction per SIMD every 4 cycles
        res["wave_instruction_slots_per_term"] = (SIMDS * CLOCK_HZ / 4.0) * 64.0 / res["atom_vector_terms_per_s"]
        out.append(res)
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", default="4096,61440")
    ap.add_argument("--n-max", default="8,16,32")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    a = mio.load_nist_fixture(4, "unwrapped")
    reps = [int(r) for r in args.replicas.split(",")]
    n_maxes = [int(v) for v in args.n_max.split(",")]
    if args.calls:
        b = make_batch(a, reps[0])
        ms = [timed(lambda: b.structure_factor(n_maxes[0]))[0] for _ in range(args.calls)]
        b.close()
        print(json.dumps({"replicas": reps[0], "n_max": n_maxes[0], "ms": ms}))
        return
    sizes = []
    for r in reps:
        sizes += one_size(a, r, n_maxes, args.rounds)
    res = {"bench": "structure_factor", "system": "SPC/E, NIST configuration 4", "sizes": sizes}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
