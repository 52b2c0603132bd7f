#!/usr/bin/env python3
"""Structure of SPC/E water from R NVT chains as examples/nvt_spce.py runs them (Loop(),
Ewald/main.jl:460-696): after equilibration, once per sweep, the six site-site pair histograms of
every replica (mmc_batch_rdf_sites, per replica) and its total dipole moment (mmc_batch_dipoles).
The chains are not disturbed.

    python3 examples/structure_spce.py [--replicas 64] [--equil 20] [--sweeps 40] [--bins 200]

Prints the position and height of the first peak of g_OO, g_OH and g_HH with the standard error over
chains (each chain's own histogram gives its own peak), and the static dielectric constant from the
fluctuation of M under the Ewald sum's conducting boundary, with its error over chains.  No
assertion on the values: runs this short are far from converged for the dielectric constant.  Needs
an MI355X.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import io as mio, observables, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402


def first_peak(r, g, r_lo, r_hi):
    """(position, height) of the largest g in [r_lo, r_hi]."""
    sel = np.nonzero((r >= r_lo) & (r <= r_hi))[0]
    k = sel[np.argmax(g[sel])]
    return r[k], g[k]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=64)
    ap.add_argument("--equil", type=int, default=20, help="sweeps before sampling")
    ap.add_argument("--sweeps", type=int, default=40, help="sampled sweeps")
    ap.add_argument("--bins", type=int, default=200)
    ap.add_argument("--temperature", type=float, default=298.15)
    args = ap.parse_args()
    T, R = args.temperature, args.replicas

    a = mio.load_nist_fixture(4, "unwrapped")
    n_mol, box, r_cut = a["com"].shape[0], a["box"], 10.0
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box,
              5.6 / box, structs.factor, r_cut, r_cut)
    b.set_option("device_moves", 1)
    tot = b.potential_ewald()
    chains = b.new_chains([t["energy"] for t in tot], [t["virial"] for t in tot],
                          dr_max=0.316555789, dphi_max=0.05)
    b.run_chains(chains, args.equil * n_mol, T, seed=11234, adjust=True, n_threads=2)
    hist = np.zeros((R, 6, args.bins + 1), dtype=np.uint64)
    M = np.zeros((args.sweeps, R, 3))
    for s in range(args.sweeps):
        b.run_chains(chains, n_mol, T, seed=20000 + s, adjust=False, n_threads=2)
        hist += b.rdf_sites(args.bins, per_replica=True)
        M[s] = b.dipoles()
    b.close()

    dr = box / 2 / args.bins
    rows, counts = observables.fold_by_type(hist, ("O", "H", "H"))
    windows = {("O", "O"): (2.2, 3.6), ("H", "O"): (1.4, 2.4), ("H", "H"): (1.8, 3.0)}
    print(f"{R} chains, {args.sweeps} sampled sweeps of {n_mol} molecules, T = {T} K, L = {box} A")
    for key in (("O", "O"), ("H", "O"), ("H", "H")):
        n_pairs = counts[key] * n_mol * (n_mol - 1) / 2
        r, g = observables.normalize_rdf_pairs(rows[key], n_pairs, dr, args.sweeps / box ** 3)   # [R, bins]
        peaks = np.array([first_peak(r, g[c], *windows[key]) for c in range(R)])
        mean, err = peaks.mean(0), peaks.std(0, ddof=1) / np.sqrt(R) if R > 1 else (np.nan, np.nan)
        print(f"g_{key[0]}{key[1]}: first peak at {mean[0]:.3f} +- {err[0]:.3f} A, "
              f"height {mean[1]:.3f} +- {err[1]:.3f}")
    eps = np.array([observables.dielectric_constant(M[:, c], T, box ** 3, structs.factor) for c in range(R)])
    err = eps.std(ddof=1) / np.sqrt(R) if R > 1 else float("nan")
    print(f"dielectric constant: {eps.mean():.1f} +- {err:.1f} over chains "
          f"(all chains pooled: {observables.dielectric_constant(M.reshape(-1, 3), T, box ** 3, structs.factor):.1f})")


if __name__ == "__main__":
    main()
