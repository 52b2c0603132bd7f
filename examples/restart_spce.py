#!/usr/bin/env python3
"""Stop a tempering run and pick it up again: Batch.save / Batch.load on NIST configuration 4
(750 molecules of SPC/E water), ladders between 260 K and 400 K.

    python3 examples/restart_spce.py [--ladders 8] [--rungs 8] [--rounds 6] [--steps 200] [--file PATH]

The uninterrupted run does 2 x `--rounds` rounds of `--steps` moves and one exchange each on one
batch.  The interrupted run does `--rounds` rounds, saves a checkpoint and destroys its batch -- what
the first process of a long run would do -- then a NEW batch, created from the starting
configuration and knowing nothing of the first, loads the checkpoint and does the other `--rounds`
rounds, as a second process would.  The caller's arrays (running energies, rungs, exchange counters,
the round) travel in the checkpoint's `extra`.  Prints whether the final energies, rungs and
temperatures of the two runs are equal bit for bit.  Needs an MI355X.
"""
import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import checkpoint, io as mio, moves, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402

DR, DPHI, R_CUT = 0.316555789, 0.05, 10.0


def new_batch(a, R):
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"], 5.6 / a["box"],
              structs.factor, R_CUT, R_CUT)
    b.set_option("device_moves", 1)      # options are not part of a checkpoint: every process sets its own
    return b


def rounds(b, c, args):
    c["energies"], _, c["attempt"], c["accept"] = b.run_exchange(
        args.rounds, args.steps, DR, DPHI, args.seed, c["energies"], c["rung"], args.rungs, round0=int(c["round"]),
        attempt=c["attempt"], accept=c["accept"], n_threads=2)
    c["round"] = np.array(int(c["round"]) + args.rounds)


def start(b, args, R):
    b.set_temperatures(np.tile(moves.geometric_ladder(260.0, 400.0, args.rungs), args.ladders))
    return dict(energies=b.potential_ewald(as_array=True)["energy"].copy(), rung=moves.initial_rungs(R, args.rungs),
                attempt=np.zeros(args.rungs - 1, dtype=np.int64), accept=np.zeros(args.rungs - 1, dtype=np.int64),
                round=np.array(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ladders", type=int, default=8)
    ap.add_argument("--rungs", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=6, help="rounds before and after the interruption")
    ap.add_argument("--steps", type=int, default=200, help="trial moves per replica and round")
    ap.add_argument("--seed", type=int, default=4711)
    ap.add_argument("--file", default=None, help="the checkpoint (default: a temporary file, removed)")
    args = ap.parse_args()
    a = mio.load_nist_fixture(4, "unwrapped")
    R = args.ladders * args.rungs
    path = args.file or os.path.join(tempfile.mkdtemp(), "restart_spce.ckpt")

    with new_batch(a, R) as b:                                   # the uninterrupted run
        whole = start(b, args, R)
        rounds(b, whole, args)
        rounds(b, whole, args)
        whole["temperatures"] = b.temperatures()

    with new_batch(a, R) as b:                                   # the first process ...
        c = start(b, args, R)
        rounds(b, c, args)
        b.save(path, extra=c)
    head = checkpoint.read_header(path)
    print(f"checkpoint: {head['n_records']} replicas x {head['record_bytes']} bytes after "
          f"{head['info']['steps_done']} steps, {os.path.getsize(path) / 2 ** 20:.1f} MiB")
    with new_batch(a, R) as b:                                   # ... and the second
        c = b.load(path)
        rounds(b, c, args)
        c["temperatures"] = b.temperatures()
    if not args.file:
        os.remove(path)
        os.rmdir(os.path.dirname(path))

    same = {k: np.asarray(whole[k]).tobytes() == np.asarray(c[k]).tobytes() for k in whole}
    print(f"after {2 * args.rounds} rounds: <E>/N = {whole['energies'].mean() / a['com'].shape[0]:.3f} K, "
          f"{int(whole['accept'].sum())} of {int(whole['attempt'].sum())} exchanges accepted")
    print("interrupted and uninterrupted run, bit for bit: "
          + ", ".join(f"{k} {'equal' if v else 'DIFFERENT'}" for k, v in same.items()))
    print("final energies equal" if same["energies"] else "final energies DIFFER")
    return 0 if all(same.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
