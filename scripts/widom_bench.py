#!/usr/bin/env python3
"""Widom insertion rates on one GPU (mmc_batch_widom), two workloads:

  - 750-molecule SPC/E (NIST config 4), R = 61 440 replicas, M = 8 insertions per replica per call:
    insertions / s; in the same process the trial moves / s of Batch.run in bench.py's default
    mode (device-drawn moves, two groups, one host thread) on the same batch, and the ratio;
  - one 10 000-molecule SPC/E replica (BASELINE configs[3]'s lattice), M = 61 440 per call:
    us per call and insertions / s.

Each figure: a warm-up, then calls (every one synchronous: it returns after the device is done)
until at least --seconds have passed, repeated --reps times; the JSON line has every repetition
and their median.

    python3 scripts/widom_bench.py [--replicas 61440] [--reps 3] [--seconds 1.0] [--out FILE]
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


def make(a, R):
    box = float(a["box"])
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, 5.6 / box,
              structs.factor, RCUT, RCUT)
    b.set_option("device_moves", 1)
    b.potential_ewald(as_array=True)   # builds S(k)
    return b


def lattice(n_mol):
    box, com, coords = mio.cubic_lattice_water(n_mol, 0.033101144, "spce", seed=11234)
    tab = structs.Tables([mio.SPCE_EPS_O, 0.0], [mio.SPCE_SIGMA_O, 0.0])
    return dict(com=com, coords=coords, atype=np.tile([1, 2, 2], n_mol),
                charge=np.tile([mio.SPCE_Q_O, mio.SPCE_Q_H, mio.SPCE_Q_H], n_mol),
                eps=tab.eps_ij, sig=tab.sig_ij, box=box)


def time_widom(b, M, seconds, reps):
    """[(calls, seconds)] of repeated mmc_batch_widom calls."""
    bs, no = np.zeros(b.R), np.zeros(b.R, dtype=np.int64)
    draw = 0
    for _ in range(3):                 # warm-up (first-call allocation, code load)
        b.widom(M, T, seed=5, draw0=draw, boltz_sum=bs, n_overlap=no)
        draw += M
    out = []
    for _ in range(reps):
        n, t0 = 0, time.perf_counter()
        while True:
            b.widom(M, T, seed=5, draw0=draw, boltz_sum=bs, n_overlap=no)
            draw += M
            n += 1
            dt = time.perf_counter() - t0
            if dt >= seconds:
                break
        out.append((n, dt))
    assert np.all(np.isfinite(bs))
    return out


def time_moves(b, seconds, reps):
    """[(moves, seconds)] of Batch.run in bench.py's default mode."""
    e = b.potential_ewald(as_array=True)["energy"].copy()
    e, _ = b.run(64, T, DR, DPHI, seed=11, energies=e, n_groups=2, n_threads=1)
    steps = 600
    out = []
    for k in range(reps):
        moves, t0 = 0, time.perf_counter()
        while True:
            e, st = b.run(steps, T, DR, DPHI, seed=12 + k, energies=e, n_groups=2, n_threads=1)
            moves += st["moves"]
            dt = time.perf_counter() - t0
            if dt >= seconds:
                break
        out.append((moves, dt))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=61440)
    ap.add_argument("--insert", type=int, default=8, help="insertions per replica per call")
    ap.add_argument("--big-insert", type=int, default=61440, help="insertions per call, 10 000 molecules")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    a = mio.load_nist_fixture(4, "unwrapped")
    b = make(a, args.replicas)
    w = time_widom(b, args.insert, args.seconds, args.reps)
    ins = [n * args.replicas * args.insert / dt for n, dt in w]
    mv = [m / dt for m, dt in time_moves(b, args.seconds, args.reps)]
    b.close()
    big = make(lattice(10000), 1)
    wb = time_widom(big, args.big_insert, args.seconds, args.reps)
    big.close()
    us = [dt / n * 1e6 for n, dt in wb]
    res = {
        "bench": "widom",
        "spce750": {"replicas": args.replicas, "insert_per_call": args.insert,
                    "insertions_per_s": ins, "insertions_per_s_median": float(np.median(ins)),
                    "trial_moves_per_s": mv, "trial_moves_per_s_median": float(np.median(mv)),
                    "ratio_median": float(np.median(ins) / np.median(mv))},
        "spce10000": {"replicas": 1, "insert_per_call": args.big_insert, "us_per_call": us,
                      "us_per_call_median": float(np.median(us)),
                      "insertions_per_s_median": float(args.big_insert / np.median(us) * 1e6)},
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
