#!/usr/bin/env python3
"""The hydrogen-bond network of SPC/E water from R NVT chains as examples/nvt_spce.py runs them
(Loop(), Ewald/main.jl:460-696): after equilibration, once per sweep, the bond graph of every replica
under eight bond criteria at once -- O-O closer than r_hb = 2.9 .. 3.6 A, H-O...O angle within 30
degrees (mmc_batch_hbond_network, one call) -- and, in a second call, the "patches" of four-bonded
molecules at 3.5 A (Stanley and Teixeira, J. Chem. Phys. 73, 3404, 1980).  The chains are not
disturbed.

    python3 examples/hbond_network_spce.py [--replicas 64] [--equil 20] [--sweeps 20]

Prints, against r_hb: the bonds per molecule, the probability that a replica's network wraps the
periodic box along at least one axis and along all three, the gel fraction (the largest wrapping
cluster over the molecules) and the mean size of the finite clusters; then the patches.  In short
runs from the fixture the network starts to wrap between 3.0 and 3.1 A, where the mean finite size
peaks.  No assertion on the values.  Needs an MI355X.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import io as mio, observables, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402

R_HB = (2.9, 3.0, 3.1, 3.2, 3.3, 3.4, 3.5, 3.6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=64)
    ap.add_argument("--equil", type=int, default=20, help="sweeps before sampling")
    ap.add_argument("--sweeps", type=int, default=20, help="sampled sweeps")
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
    K = len(R_HB)
    size_hist = np.zeros((K, n_mol + 1), dtype=np.uint64)
    deg_hist = np.zeros((K, 17), dtype=np.uint64)
    stats, patch_stats = [], []
    patch_hist = np.zeros((1, n_mol + 1), dtype=np.uint64)
    for s in range(args.sweeps):
        b.run_chains(chains, n_mol, T, seed=20000 + s, adjust=False, n_threads=2)
        out = b.hbond_network(R_HB, 30.0, 0)
        size_hist += out["size_hist"]
        deg_hist += out["deg_hist"]
        stats.append(out["stats"])
        out = b.hbond_network(3.5, 30.0, 4)
        patch_hist += out["size_hist"]
        patch_stats.append(out["stats"])
    b.close()
    stats, patch_stats = np.concatenate(stats), np.concatenate(patch_stats)   # [sweeps R, K, 8]: every frame a sample

    print(f"{R} chains, {args.sweeps} sampled sweeps of {n_mol} molecules, T = {T} K, L = {box} A, 30 degrees")
    print(f"flagged frames (a molecule with more than 16 bonds): {int(stats[..., 7].sum())}")
    p_any, p_all = observables.percolation_probability(stats)
    gel = np.nanmean(observables.gel_fraction(stats), axis=0)
    mean_s = observables.mean_cluster_size(size_hist, stats)
    f = observables.bond_fractions(deg_hist)
    n_hb = (f * np.arange(17.0)).sum(-1)
    print(" r_hb   bonds/mol  f_4     P(wraps)  P(x,y,z)  gel     <S finite>")
    for k, r in enumerate(R_HB):
        print(f" {r:4.2f}   {n_hb[k]:8.3f}  {f[k, 4]:.3f}   {p_any[k]:7.3f}   {p_all[k]:7.3f}   {gel[k]:.3f}   {mean_s[k]:9.2f}")
    n_s, w_s = observables.cluster_size_distribution(patch_hist)
    sites = patch_stats[:, 0, 1]
    print(f"four-bonded molecules at 3.5 A: {sites.mean():.1f} of {n_mol} per frame in "
          f"{patch_stats[:, 0, 2].mean():.1f} patches; largest {patch_stats[:, 0, 3].max()}, "
          f"mean size {(patch_stats[:, 0, 1].sum() / max(patch_stats[:, 0, 2].sum(), 1)):.2f}, "
          f"wrapping frames {int((patch_stats[:, 0, 5] != 0).sum())}")
    top = np.flatnonzero(n_s[0])[:8]
    print("patches by size s: " + " ".join(f"{s}:{w_s[0, s]:.3f}" for s in top) + "  (share of the four-bonded molecules)")


if __name__ == "__main__":
    main()
