#!/usr/bin/env python3
"""One bond_order call (Steinhardt q_l, bond correlations, solid-like molecules and their clusters,
mmc_batch_bond_order) against one shell_order() call and one local_order(400) call, on one GPU, one
process: 750-molecule SPC/E (NIST config 4) after 64 moves, at bench.py's headline replica count.

Per size, after a warm-up of every side, --rounds rounds of
  chill      bond_order with its defaults (CHILL+: l = 3, four neighbours inside 3.5 A, staggered and
             eclipsed windows, 200 + 200 bins), every summed output and the sums: all three phases;
  q6         l = 6 with 16 neighbours inside 3.5 A, a q6 criterion (A = [0.5, 1], min_a = 7): the
             longest harmonics and the largest records;
  phase_a    the neighbour phase alone: the defaults with only q_hist asked for (scan, sort,
             harmonics, q_lm and the records; no k_bond_corr, no k_bond_clusters);
  phase_ab   the first two phases: q_hist, qbar_hist, c_hist and ab_hist, no clusters;
  shell      one shell_order() call with its defaults: the same scan and sort;
  local      one local_order(400) call, summed output: the yardstick of the other passes,
taken in turn (chill, q6, ..., local, chill, ...) so that drift hits all alike.  Every call is
synchronous: it returns after the device is done and the output is on the host.  The JSON has every
sample, medians and the spread (min, max), the ratios to shell_order and local_order, the chunk
(replicas per chunk under the 256 MiB scratch budget) and the frame's solid fraction, largest nucleus
and <q_l>.  Not measured: hardware counters, the per-replica histograms, the detail outputs.

    python3 scripts/bond_order_bench.py [--replicas 61440] [--rounds 7] [--chunk 0] [--out profiles/bond_order_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import _lib, io as mio, observables as obs, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402

T, DR, DPHI, RCUT = 298.15, 0.316555789, 0.05, 10.0
Q_BINS = 400
INF = float("inf")
DEFAULTS = dict(l=3, r_nb=3.5, n_nb=4, a=(-INF, -0.8), b=(-0.35, 0.25), min_a=3, min_ab=4, q_bins=200, c_bins=200)
Q6 = dict(DEFAULTS, l=6, n_nb=16, a=(0.5, 1.0), min_a=7, min_ab=0)
HISTS = ("q_hist", "qbar_hist", "c_hist", "ab_hist", "size_hist")
SCRATCH_BYTES = 256 << 20           # BO_SCRATCH_BYTES of csrc/mmc_bondorder.inc
RECORD_BYTES = 8 * 16 + 4 * 16 + 4 + 1


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    return {"ms": ms, "median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def partial_call(b, want, **kw):
    """The C call with only the summed histograms named in `want`."""
    p = dict(DEFAULTS, **kw)
    shape = dict(q_hist=(p["q_bins"] + 1,), qbar_hist=(p["q_bins"] + 1,), c_hist=(p["c_bins"] + 1,), ab_hist=(17, 17),
                 size_hist=(b.n_mol + 1,))
    res = {k: np.zeros(shape[k], dtype=np.uint64) for k in HISTS if k in want}
    u64 = C.POINTER(C.c_uint64)
    _lib.check(_lib.lib().mmc_batch_bond_order(
        b._h, p["l"], p["r_nb"], p["n_nb"], p["a"][0], p["a"][1], p["b"][0], p["b"][1], p["min_a"], p["min_ab"],
        p["q_bins"], p["c_bins"], 0, *[res[k].ctypes.data_as(u64) if k in res else None for k in HISTS],
        None, None, None, None, None, None, None))
    return res


def one_size(a, R, rounds, chunk):
    box = float(a["box"])
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, 5.6 / box,
              structs.factor, RCUT, RCUT)
    b.set_option("device_moves", 1)
    b.set_option("bond_chunk", chunk)
    e = b.potential_ewald(as_array=True)["energy"].copy()
    e, _ = b.run(64, T, DR, DPHI, seed=11, energies=e, n_groups=2, n_threads=1)   # replicas diverge

    sides = {
        "chill": lambda: b.bond_order(),
        "q6": lambda: b.bond_order(**Q6),
        "phase_a": lambda: partial_call(b, ("q_hist",)),
        "phase_ab": lambda: partial_call(b, HISTS[:4]),
        "shell": lambda: b.shell_order(),
        "local": lambda: b.local_order(Q_BINS),
    }
    out = {}
    for _ in range(2):                      # warm-up: code load, first allocations
        for k, fn in sides.items():
            out[k] = fn()
    n = a["com"].shape[0]
    bo = out["chill"]
    assert bo["q_hist"].sum() == R * n and np.all(bo["stats"][:, :3].sum(1) == n)
    assert np.array_equal(out["phase_a"]["q_hist"], bo["q_hist"])
    assert all(np.array_equal(out["phase_ab"][k], bo[k]) for k in HISTS[:4])
    ms = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            ms[k].append(timed(fn)[0])
    b.close()
    n_chunk = chunk if chunk > 0 else SCRATCH_BYTES // ((RECORD_BYTES + 16) * n)      # + q_l and qbar_l for the sums
    res = {"replicas": R, "n_mol": int(n), "defaults": {k: list(v) if isinstance(v, tuple) else v for k, v in DEFAULTS.items()},
           "q6": {k: list(v) if isinstance(v, tuple) else v for k, v in Q6.items()},
           "replicas_per_chunk": int(min(n_chunk, R)), "scratch_budget_bytes": SCRATCH_BYTES, "q_bins_local": Q_BINS}
    res.update({k: summary(v) for k, v in ms.items()})
    med = {k: res[k]["median_ms"] for k in sides}
    s6 = out["q6"]
    res.update(chill_over_shell=med["chill"] / med["shell"], chill_over_local=med["chill"] / med["local"],
               q6_over_shell=med["q6"] / med["shell"], q6_over_local=med["q6"] / med["local"],
               phase_a_over_shell=med["phase_a"] / med["shell"], phase_a_over_local=med["phase_a"] / med["local"],
               phase_a_share_of_chill=med["phase_a"] / med["chill"], phase_ab_share_of_chill=med["phase_ab"] / med["chill"],
               solid_fraction=float(obs.solid_fraction(bo["stats"].sum(0))),
               largest_nucleus=int(obs.largest_nucleus(bo["stats"]).max()),
               q3_mean=float(bo["sums"][:, 0].sum() / bo["sums"][:, 1].sum()),
               q6_mean=float(s6["sums"][:, 0].sum() / s6["sums"][:, 1].sum()),
               q6_solid_fraction=float(obs.solid_fraction(s6["stats"].sum(0))),
               truncated=int(bo["stats"][:, 3].sum()), flagged=int(bo["stats"][:, 2].sum()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", default="61440")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=0, help="option bond_chunk (0: by the scratch budget)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    a = mio.load_nist_fixture(4, "unwrapped")
    res = {"bench": "bond_order", "system": "SPC/E, NIST configuration 4",
           "sizes": [one_size(a, int(r), args.rounds, args.chunk) for r in args.replicas.split(",")]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
