#!/usr/bin/env python3
"""Parallel tempering of SPC/E water: ladders of replicas between 260 K and 400 K that exchange
temperatures (Batch.set_temperatures, Batch.run_exchange), NIST configuration 4 (750 molecules).

    python3 examples/tempering_spce.py [--ladders 16] [--rungs 16] [--equil 20] [--rounds 200] [--steps 750]

Every ladder is an independent replica-exchange run; replica r of a ladder starts on rung r.  After
the equilibration sweeps (no exchanges) it runs `--rounds` rounds of `--steps` trial moves and one
exchange each, alternating even and odd pairs, and prints per neighbouring pair of rungs the
acceptance ratio, per rung <E>/N with its standard error over the ladders and
C_v / (N k_B) = (<E^2> - <E>^2) / (N T^2) from the energy fluctuation (the configurational part),
and the completed bottom -> top -> bottom journeys of the replicas.  Nothing is asserted: runs this
short are not converged at the cold end.  Needs an MI355X.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import io as mio, moves, observables, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ladders", type=int, default=16)
    ap.add_argument("--rungs", type=int, default=16)
    ap.add_argument("--t-lo", type=float, default=260.0)
    ap.add_argument("--t-hi", type=float, default=400.0)
    ap.add_argument("--equil", type=int, default=20, help="sweeps before the first exchange")
    ap.add_argument("--rounds", type=int, default=200, help="rounds of moves + one exchange")
    ap.add_argument("--steps", type=int, default=750, help="trial moves per replica and round")
    ap.add_argument("--seed", type=int, default=11234)
    args = ap.parse_args()
    a = mio.load_nist_fixture(4, "unwrapped")
    n_mol, box, r_cut, n = a["com"].shape[0], a["box"], 10.0, args.rungs
    R = args.ladders * n
    ladder = moves.geometric_ladder(args.t_lo, args.t_hi, n)
    print(f"{args.ladders} ladders of {n} rungs, {args.t_lo} ... {args.t_hi} K; {args.equil} sweeps, then "
          f"{args.rounds} rounds of {args.steps} moves and one exchange; {n_mol} molecules, L = {box} A")
    dr, dphi = 0.316555789, 0.05
    with Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, 5.6 / box,
               structs.factor, r_cut, r_cut) as b:
        b.set_option("device_moves", 1)
        b.set_temperatures(np.tile(ladder, args.ladders))
        rung = moves.initial_rungs(R, n)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        e, _ = b.run(args.equil * n_mol, ladder[0], dr, dphi, seed=args.seed, energies=e, n_threads=2)
        attempt = accept = None
        e_sum, e2_sum, history = np.zeros((n, args.ladders)), np.zeros((n, args.ladders)), [rung.copy()]
        for k in range(args.rounds):      # one round per call, so that every round's energies can be sampled
            held = rung.copy()            # (the rungs the round's moves ran on: the exchange comes after them)
            e, st, attempt, accept = b.run_exchange(1, args.steps, dr, dphi, args.seed + 1, e, rung, n, round0=k,
                                                    attempt=attempt, accept=accept, n_threads=2)
            g = observables.by_rung(e, held, n)
            e_sum += g
            e2_sum += g * g
            history.append(rung.copy())
        drift = np.abs(e - b.potential_ewald(as_array=True)["energy"]).max()
    ratio = observables.exchange_acceptance(attempt, accept)
    trips = observables.round_trips(np.array(history), n_rungs=n)
    mean = e_sum / args.rounds                                  # [rung, ladder]: every ladder's own average
    var = e2_sum / args.rounds - mean * mean
    print(" rung    T / K    <E>/N / K      +-     C_v/(N k_B)   swap with the next")
    for k in range(n):
        err = mean[k].std(ddof=1) / np.sqrt(args.ladders) / n_mol if args.ladders > 1 else float("nan")
        swap = f"{ratio[k]:.3f}" if k + 1 < n else ""
        print(f"{k:5d} {ladder[k]:8.2f} {mean[k].mean() / n_mol:12.3f} {err:9.3f} "
              f"{var[k].mean() / (n_mol * ladder[k] ** 2):12.3f}   {swap}")
    print(f"round trips: {int(trips.sum())} in all, at most {int(trips.max())} by one replica, "
          f"{int((trips > 0).sum())} of {R} replicas completed one   (running total vs recompute: {drift:.2e} K)")


if __name__ == "__main__":
    main()
