#!/usr/bin/env python3
"""Where the dielectric constant of SPC/E water comes from: the distance-dependent Kirkwood factor
G_K(r) and the orientational projections h110(r) and h112(r) of R NVT chains as
examples/nvt_spce.py runs them (Loop(), Ewald/main.jl:460-696).  After equilibration the chains run
in blocks of sweeps; between the blocks every replica's orientational pair correlations
(mmc_batch_orient_corr, per replica) and its total dipole moment (mmc_batch_dipoles) are taken.  The
chains are not disturbed.

    python3 examples/kirkwood_spce.py [--replicas 64] [--equil 20] [--blocks 40] [--sweeps 1] [--bins 60]

Prints G_K, h110 and h112 (and g_OO, <P2>) on a few radii with the standard error over chains, then
the whole-box G_K = <|sum_i u_i|^2> / N beside the dielectric constant from the fluctuation of M
under the Ewald sum's conducting boundary.  With a rigid model |mu| is the same for every molecule,
so (eps - 1) 3 V T / (4 pi factor N mu^2) is the whole-box G_K again, up to <M>^2: the last line
prints both sides.  No assertion on the values: runs this short are far from converged for either.
Needs an MI355X.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import io as mio, observables, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402


def mean_err(x):
    """Mean and standard error over the leading (chain) axis."""
    x = np.asarray(x, dtype=float)
    err = x.std(0, ddof=1) / np.sqrt(x.shape[0]) if x.shape[0] > 1 else np.full(x.shape[1:], np.nan)
    return x.mean(0), err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=64)
    ap.add_argument("--equil", type=int, default=20, help="sweeps before sampling")
    ap.add_argument("--blocks", type=int, default=40, help="sampled frames")
    ap.add_argument("--sweeps", type=int, default=1, help="sweeps per block")
    ap.add_argument("--bins", type=int, default=60)
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
    hist = np.zeros((R, 4, args.bins + 2), dtype=np.int64)
    M = np.zeros((args.blocks, R, 3))
    for s in range(args.blocks):
        b.run_chains(chains, args.sweeps * n_mol, T, seed=20000 + s, adjust=False, n_threads=2)
        hist += b.orient_corr(args.bins, per_replica=True)      # bins of (L / 2) / bins, the rest in the last slot
        M[s] = b.dipoles()
    b.close()

    dr = box / 2 / args.bins
    gk, gk_err = mean_err(observables.kirkwood_gk(hist, n_mol, args.blocks))                  # [bins + 2]
    r, g, h110, h112, p2 = observables.orient_projections(hist, n_mol, dr, args.blocks / box ** 3)
    print(f"{R} chains, {args.blocks} frames {args.sweeps} sweep(s) apart, {n_mol} molecules, T = {T} K, L = {box} A")
    print("   r / A    g_OO            h110              h112              <P2>              G_K(r + dr/2)")
    cols = [mean_err(x) for x in (g, h110, h112, p2)]
    for k in range(max(args.bins // 15, 1) - 1, args.bins, max(args.bins // 15, 1)):
        line = f"{r[k]:8.3f}"
        for m, e in cols:
            line += f"  {m[k]:8.4f} +- {e[k]:6.4f}"
        print(line + f"  {gk[k + 1]:8.4f} +- {gk_err[k + 1]:6.4f}")
    print(f"G_K at L/2 = {gk[-2]:.3f} +- {gk_err[-2]:.3f};  whole box <|sum u|^2> / N = {gk[-1]:.3f} +- {gk_err[-1]:.3f}")

    eps = np.array([observables.dielectric_constant(M[:, c], T, box ** 3, structs.factor) for c in range(R)])
    eps_m, eps_e = mean_err(eps)
    # one molecule's dipole: rigid, so the same for all (e A)
    d = a["coords"][:3] - a["com"][0]
    d -= box * np.round(d / box)
    mu2 = float(((a["charge"][:3, None] * d).sum(0) ** 2).sum())
    y = 4.0 * np.pi * structs.factor * n_mol * mu2 / (3.0 * box ** 3 * T)
    print(f"dielectric constant from <M^2> - <M>^2: {eps_m:.1f} +- {eps_e:.1f} over chains;  "
          f"(eps - 1) / (4 pi factor N mu^2 / (3 V T)) = {(eps_m - 1) / y:.3f},  whole-box G_K = {gk[-1]:.3f} "
          f"(they differ by <M>^2 / (N mu^2), which vanishes only for a converged run)")


if __name__ == "__main__":
    main()
