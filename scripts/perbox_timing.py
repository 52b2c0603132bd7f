#!/usr/bin/env python3
"""Cost of per-replica boxes (mmc_batch_set_boxes) on one GPU, 750-molecule SPC/E (NIST config 4):

  - trial moves / s of a per-box batch (kernel 1 with each replica's table staged in LDS, moves
    drawn by k_propose with each replica's box) against the SAME batch in NVT with one box and
    kernel 1 (option "kernel" = 1, device moves, no move server);
  - ms per batched volume move: mmc_batch_volume_trial_replicas (every replica moves) followed by
    mmc_batch_volume_settle (every replica rejected), host wall clock.

    python3 scripts/perbox_timing.py [--replicas 32,256] [--steps 750] [--reps 5] [--out FILE]

One JSON line per R on stdout (and in FILE).  Numbers, not a gate.
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

T, DR, DPHI, ALPHA, RCUT = 298.15, 0.316555789, 0.05, 5.6, 10.0


def make(a, R):
    box = float(a["box"])
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, ALPHA / box,
              structs.factor, RCUT, RCUT)
    b.set_option("device_moves", 1)
    b.set_option("persistent", 0)
    b.set_option("kernel", 1)
    return b


def moves_per_s(b, steps, reps, seed):
    e = b.potential_ewald(as_array=True)["energy"].copy()
    e, _ = b.run(steps, T, DR, DPHI, seed=seed, energies=e)            # warm-up
    best = 0.0
    for k in range(reps):
        e, st = b.run(steps, T, DR, DPHI, seed=seed + 1 + k, energies=e)
        best = max(best, st["moves"] / (st["wall_ms"] * 1e-3))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", default="32,256")
    ap.add_argument("--steps", type=int, default=750)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    a = mio.load_nist_fixture(4, "unwrapped")
    box = float(a["box"])
    lines = []
    for R in [int(x) for x in args.replicas.split(",")]:
        with make(a, R) as nvt:
            m_nvt = moves_per_s(nvt, args.steps, args.reps, 101)
        with make(a, R) as b:
            boxes = box * np.linspace(0.99, 1.01, R)
            for r in range(R):   # each replica rescaled to its box on the host (volumeChange.jl:62-80)
                f = boxes[r] / box
                com = a["com"] * f
                b.set_replica(r, com, a["coords"] + np.repeat(com - a["com"], 3, axis=0))
            b.set_boxes(boxes, ALPHA)
            b.recip_long()
            m_pb = moves_per_s(b, args.steps, args.reps, 101)
            new = boxes * 1.002
            b.volume_trial_replicas(new)                               # warm-up (allocates the snapshot)
            b.volume_settle(np.zeros(R, dtype=np.int32))
            ms = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                b.volume_trial_replicas(new)
                b.volume_settle(np.zeros(R, dtype=np.int32))
                ms.append((time.perf_counter() - t0) * 1e3)
        line = dict(replicas=R, molecules=int(a["com"].shape[0]), steps=args.steps,
                    nvt_kernel1_moves_per_s=m_nvt, per_box_moves_per_s=m_pb,
                    per_box_over_nvt=m_pb / m_nvt, batched_volume_move_ms=float(np.median(ms)),
                    batched_volume_move_ms_min=float(np.min(ms)))
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
