#!/usr/bin/env python3
"""SPC/E water in reciprocal space: the partial structure factors S_OO(q), S_OH(q), S_HH(q), the
charge structure factor S_ZZ(q) and the longitudinal dielectric response 1 - 1 / eps_L(q) on the
box's own wave vectors, from R NVT chains as examples/nvt_spce.py runs them (Loop(),
Ewald/main.jl:460-696).  After equilibration the chains run in blocks of sweeps; between the blocks
every replica's slot-density products are taken (mmc_batch_structure_factor, summed over the
replicas).  The chains are not disturbed.

    python3 examples/structure_factor_spce.py [--replicas 64] [--equil 20] [--blocks 40] [--sweeps 1] [--n-max 8] [--shells 12]

Prints q, S_OO, S_OH, S_HH, S_ZZ and 1 - 1 / eps_L of the lowest shells.  S_OO(q -> 0) tends to
rho k_B T kappa_T, and 1 - 1 / eps_L to 1 - 1 / eps.  No assertion on the values: runs this short
are far from converged at the lowest q.  Needs an MI355X.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import io as mio, observables, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=64)
    ap.add_argument("--equil", type=int, default=20, help="sweeps before sampling")
    ap.add_argument("--blocks", type=int, default=40, help="sampled frames per chain")
    ap.add_argument("--sweeps", type=int, default=1, help="sweeps per block")
    ap.add_argument("--n-max", type=int, default=8, help="vectors up to |n| <= n_max (at most 32)")
    ap.add_argument("--shells", type=int, default=12, help="shells printed")
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
    sq = np.zeros((6, args.n_max ** 2 + 1))
    for s in range(args.blocks):
        b.run_chains(chains, args.sweeps * n_mol, T, seed=20000 + s, adjust=False, n_threads=2)
        count, frame = b.structure_factor(args.n_max)           # summed over the replicas
        sq += frame
    b.close()

    frames = args.blocks * R
    shell, cnt, q = observables.structure_factor_shells(args.n_max, box)
    part = observables.partial_structure_factors(sq, count, n_mol, ("O", "H", "H"), n_frames=frames)
    szz = observables.charge_structure_factor(sq, count, a["charge"][:3], n_mol, n_frames=frames)
    resp = observables.dielectric_longitudinal(szz, q, n_mol, box ** 3, T, structs.factor)
    print(f"{R} chains, {args.blocks} frames {args.sweeps} sweep(s) apart, {n_mol} molecules, T = {T} K, L = {box} A")
    print("  |n|^2  vectors   q / A^-1      S_OO      S_OH      S_HH        S_ZZ   1 - 1/eps_L")
    for k in range(min(args.shells, shell.size)):
        print(f"{shell[k]:7d} {cnt[k]:8d} {q[k]:11.4f} {part[('O', 'O')][k]:9.4f} {part[('H', 'O')][k]:9.4f} "
              f"{part[('H', 'H')][k]:9.4f} {szz[k]:11.6f} {resp[k]:13.4f}")
    print(f"largest q = {q[-1]:.3f} A^-1: S_OO = {part[('O', 'O')][-1]:.4f}, S_HH = {part[('H', 'H')][-1]:.4f}")


if __name__ == "__main__":
    main()
