#!/usr/bin/env python3
"""The ring statistics of the hydrogen-bond network of SPC/E water from R NVT chains as
examples/nvt_spce.py runs them (Loop(), Ewald/main.jl:460-696): after equilibration, once per sweep,
the shortest-path rings (Franzblau, Phys. Rev. B 44, 4925, 1991; counted in water by Matsumoto, Baba
and Ohmine, J. Chem. Phys. 127, 134504, 2007) of 3 to 8 molecules in the bond graph of every replica
-- O-O closer than 3.5 A, H-O...O angle within 30 degrees (mmc_batch_hbond_rings, one call).  The
chains are not disturbed.

    python3 examples/hbond_rings_spce.py [--replicas 64] [--equil 20] [--sweeps 20]

Prints, by ring size: the rings per molecule, their share of all rings, the share that is homodromic
(donations running round one way), the mean number of such rings a molecule is a member of, and the
rings that close through the periodic box, which are counted apart.  Ice Ih and Ic would show two
six-rings per molecule and nothing else.  No assertion on the values.  Needs an MI355X.
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
    ap.add_argument("--sweeps", type=int, default=20, help="sampled sweeps")
    ap.add_argument("--temperature", type=float, default=298.15)
    ap.add_argument("--r-hb", type=float, default=3.5)
    ap.add_argument("--theta", type=float, default=30.0)
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
    ring_hist = np.zeros((3, 9), dtype=np.uint64)
    member_hist = np.zeros((9, 33), dtype=np.uint64)
    stats = []
    for s in range(args.sweeps):
        b.run_chains(chains, n_mol, T, seed=20000 + s, adjust=False, n_threads=2)
        out = b.hbond_rings(args.r_hb, args.theta, 8)
        ring_hist += out["ring_hist"]
        member_hist += out["member_hist"]
        stats.append(out["stats"])
    b.close()
    stats = np.concatenate(stats)                                   # [sweeps R, 8]: every frame a sample
    frames = stats.shape[0] - int(stats[:, 7].sum())

    print(f"{R} chains, {args.sweeps} sampled sweeps of {n_mol} molecules, T = {T} K, L = {box} A, "
          f"r_hb = {args.r_hb} A, {args.theta} degrees")
    print(f"flagged frames (a molecule with more than 8 bonds): {int(stats[:, 7].sum())}")
    print(f"bonds per molecule {2.0 * stats[:, 0].mean() / n_mol:.3f}, rings per frame {stats[:, 1].mean():.1f}, "
          f"molecules in no ring {stats[:, 4].mean():.1f}, most rings through one molecule {stats[:, 5].max()}")
    per_mol = observables.ring_size_distribution(ring_hist, n_mol, max(frames, 1))
    share = observables.ring_fractions(ring_hist)
    homo = observables.homodromic_fraction(ring_hist)
    member = observables.ring_membership(member_hist)
    print(" n   rings/mol   share   homodromic   memberships/mol    through the box (per frame)")
    for n in range(3, 9):
        print(f" {n}   {per_mol[n]:9.4f}   {share[n]:.3f}   {homo[n]:10.3f}   {member[n]:16.3f}   "
              f"{ring_hist[1, n] / max(frames, 1):.3f}")
    print(f"all {per_mol.sum():9.4f}                        {member[0]:16.3f}")


if __name__ == "__main__":
    main()
