#!/usr/bin/env python3
"""The picture of water's first shell: the spatial distribution functions g_O(x, y, z) and
g_H(x, y, z) of the neighbours' oxygens and hydrogens around an SPC/E molecule in its own frame
(z the H-O-H bisector, x in the molecular plane), from R NVT chains as examples/nvt_spce.py runs
them.  After equilibration the chains run in blocks of sweeps; between the blocks the counts of
every replica (mmc_batch_sdf, summed over the replicas, folded onto |x| and |y|) are added up.  The
chains are not disturbed.

    python3 examples/sdf_spce.py [--replicas 64] [--equil 20] [--blocks 40] [--sweeps 1]
                                 [--n-half 24] [--cell 0.25] [--out sdf_spce.npz]

Prints the position and height of the two maxima of g_O -- the acceptor oxygens in front of the
hydrogens (z > 0, off the axis in the molecular plane) and the donor band behind the oxygen (z < 0,
out of the plane) -- and of g_H, and saves the counts, the densities and the cell centres as .npz
(observables.sdf_unfold gives the full mirror-symmetric grids for plotting).  No assertion on the
values: runs this short are noisy.  Needs an MI355X.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import io as mio, observables, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402

FOLD = 3


def maximum(g, centres, keep):
    """Position and height of the largest value of g among the cells where keep [g_z] holds."""
    masked = np.where(keep[None, None, :], g, -1.0)
    ix, iy, iz = np.unravel_index(np.argmax(masked), g.shape)
    return (centres[0][ix], centres[1][iy], centres[2][iz]), g[ix, iy, iz]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=64)
    ap.add_argument("--equil", type=int, default=20, help="sweeps before sampling")
    ap.add_argument("--blocks", type=int, default=40, help="sampled frames")
    ap.add_argument("--sweeps", type=int, default=1, help="sweeps per block")
    ap.add_argument("--n-half", type=int, default=24)
    ap.add_argument("--cell", type=float, default=0.25)
    ap.add_argument("--temperature", type=float, default=298.15)
    ap.add_argument("--out", default="sdf_spce.npz")
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
    first = b.sdf(args.n_half, args.cell, FOLD, 1)
    counts = {"O": np.zeros_like(first.grid), "H": np.zeros_like(first.grid)}
    for s in range(args.blocks):
        b.run_chains(chains, args.sweeps * n_mol, T, seed=20000 + s, adjust=False, n_threads=2)
        counts["O"] += b.sdf(args.n_half, args.cell, FOLD, 1).grid       # slot 0: the oxygens
        counts["H"] += b.sdf(args.n_half, args.cell, FOLD, 6).grid       # slots 1 and 2: the hydrogens
    b.close()

    frames = args.blocks * R
    centres = observables.sdf_cell_centres(args.n_half, args.cell, FOLD)
    g = {"O": observables.sdf_density(counts["O"], n_mol, frames, box ** 3, args.cell, FOLD, 1),
         "H": observables.sdf_density(counts["H"], n_mol, frames, box ** 3, args.cell, FOLD, 6)}
    print(f"{R} chains, {args.blocks} frames {args.sweeps} sweep(s) apart, {n_mol} molecules, T = {T} K, "
          f"cube of {2 * args.n_half * args.cell} A in cells of {args.cell} A")
    z = centres[2]
    for name, keep, what in (("O", z > 0, "acceptor oxygens in front of the hydrogens (z > 0)"),
                             ("O", z < 0, "donor oxygens behind the oxygen (z < 0)"),
                             ("H", z > 0, "hydrogens beyond the acceptors (z > 0)"),
                             ("H", z < 0, "donated hydrogens behind the oxygen (z < 0)")):
        (x, y, zz), h = maximum(g[name], centres, keep)
        print(f"g_{name}: {what}: maximum {h:7.2f} at (|x|, |y|, z) = ({x:.3f}, {y:.3f}, {zz:.3f}) A")
    np.savez(args.out, counts_O=counts["O"], counts_H=counts["H"], g_O=g["O"], g_H=g["H"],
             x=centres[0], y=centres[1], z=centres[2], frames=frames, fold=FOLD)
    print(f"saved {args.out}")


if __name__ == "__main__":
    main()
