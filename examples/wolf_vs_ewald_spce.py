#!/usr/bin/env python3
"""SPC/E water with the Ewald sum and with the reference's Wolf summation (`Wolf = true`,
Ewald/main.jl:75), side by side: two batches of R NVT chains from the same start and the same seeds,
one per Coulomb style (Batch.set_coulomb_style).  The reference's README shows this comparison as
its proof of concept ("SPC/E water RDF - Wolf & Ewald").

    python3 examples/wolf_vs_ewald_spce.py [--replicas 64] [--equil 20] [--sweeps 20] [--bins 200]

After the equilibration sweeps it prints, for each style, <E>/N by the style's own total
(potential_ewald / potential_wolf, averaged over chains and sampled sweeps) and the position and
height of the first peak of g_OO (rdf_sites).  Nothing is asserted: the Wolf sum is an
approximation, and runs this short are not converged.  Needs an MI355X.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import io as mio, observables, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402


def run_style(style, a, args):
    n_mol, box, r_cut, R, T = a["com"].shape[0], a["box"], 10.0, args.replicas, args.temperature
    with Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box,
               5.6 / box, structs.factor, r_cut, r_cut) as b:
        b.set_option("device_moves", 1)
        b.recip_long()
        b.set_coulomb_style(style)
        total = b.potential_wolf if style == "wolf" else b.potential_ewald
        e = total(as_array=True)["energy"].copy()
        e, _ = b.run(args.equil * n_mol, T, 0.316555789, 0.05, seed=11234, energies=e, n_threads=2)
        hist = np.zeros((6, args.bins + 1), dtype=np.uint64)
        e_sum = 0.0
        for s in range(args.sweeps):
            e, _ = b.run(n_mol, T, 0.316555789, 0.05, seed=20000 + s, energies=e, n_threads=2)
            hist += b.rdf_sites(args.bins)
            e_sum += e.mean()
        drift = np.abs(e - total(as_array=True)["energy"]).max()
    rows, counts = observables.fold_by_type(hist[None], ("O", "H", "H"))
    n_pairs = counts[("O", "O")] * n_mol * (n_mol - 1) / 2
    r, g = observables.normalize_rdf_pairs(rows[("O", "O")], n_pairs, box / 2 / args.bins,
                                           args.sweeps * R / box ** 3)
    sel = np.nonzero((r >= 2.2) & (r <= 3.6))[0]
    k = sel[np.argmax(g[0][sel])]
    return e_sum / args.sweeps / n_mol, r[k], g[0][k], drift


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=64)
    ap.add_argument("--equil", type=int, default=20, help="sweeps before sampling")
    ap.add_argument("--sweeps", type=int, default=20, help="sampled sweeps")
    ap.add_argument("--bins", type=int, default=200)
    ap.add_argument("--temperature", type=float, default=298.15)
    args = ap.parse_args()
    a = mio.load_nist_fixture(4, "unwrapped")
    print(f"{args.replicas} chains per style, {args.equil} + {args.sweeps} sweeps of {a['com'].shape[0]} "
          f"molecules, T = {args.temperature} K, L = {a['box']} A")
    for style in ("ewald", "wolf"):
        e_n, r_peak, g_peak, drift = run_style(style, a, args)
        print(f"{style:5s}: <E>/N = {e_n:10.3f} K   g_OO first peak at {r_peak:.3f} A, height {g_peak:.3f}   "
              f"(running total vs recompute: {drift:.2e} K)")


if __name__ == "__main__":
    main()
