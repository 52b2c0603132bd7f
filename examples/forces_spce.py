#!/usr/bin/env python3
"""Mean-square force and torque of SPC/E water and the first-order quantum correction: R NVT chains
as examples/nvt_spce.py runs them (Loop(), Ewald/main.jl:460-696), and after every block one
mmc_batch_forces call over all molecules of every replica (read-only: the chains are not disturbed).

    python3 examples/forces_spce.py [--replicas 256] [--blocks 8] [--sweeps 10]

Prints per block <F^2>, <tau^2> and the largest |sum_i F_i| of a replica (a health check: it
vanishes up to rounding), and at the end the Wigner-Kirkwood correction to the free energy,
dA = hbar^2 / (24 (k_B T)^2) (<F^2> / M + <tau' I^-1 tau>) per molecule
(observables.quantum_correction), with its translational and rotational parts and the standard error
over the replicas.  Forces are minus the gradient of the reference's own potential(..., "ewald") at
fixed neighbour sets (include/mmc_hip.h).  No assertion on any value.  Needs an MI355X.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import io as mio, observables, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402

KJ_PER_MOL_PER_K = structs.R  # kJ mol^-1 K^-1 (energies here are E / k_B in K)
MASS = (15.9994, 1.00794, 1.00794)  # amu: O, H, H


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--sweeps", type=int, default=10, help="sweeps (N_mol trial moves) per block")
    ap.add_argument("--temperature", type=float, default=298.15)
    args = ap.parse_args()
    T, R = args.temperature, args.replicas

    a = mio.load_nist_fixture(4, "unwrapped")
    n_mol, box, r_cut = a["com"].shape[0], a["box"], 10.0
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, 5.6 / box,
              structs.factor, r_cut, r_cut)
    b.set_option("device_moves", 1)
    tot = b.potential_ewald()                                   # main.jl:408 (also builds S(k))
    chains = b.new_chains([t["energy"] for t in tot], [t["virial"] for t in tot],
                          dr_max=0.316555789, dphi_max=0.05)
    total, n_flag = np.zeros((R, 9)), np.zeros(R, dtype=np.int64)
    for blk in range(1, args.blocks + 1):
        b.run_chains(chains, args.sweeps * n_mol, T, seed=11234 + 1000 * blk, adjust=True, n_threads=2)
        res = b.forces(mass=MASS, n_flagged=n_flag)
        total += res["fsum"]
        ms = observables.mean_square_force(res["fsum"])
        print(f"block {blk:3d}: <E>/N = {chains['energy'].mean() / n_mol:9.2f} K, <F^2> = {ms['f2_pooled']:.5e} (K/A)^2, "
              f"<tau^2> = {ms['tau2_pooled']:.5e} K^2, max |sum F| = {np.abs(res['fsum'][:, 4:7]).max():.2e} K/A, "
              f"flagged {int(n_flag.sum())}")
    b.close()

    ms = observables.mean_square_force(total)
    qc = observables.quantum_correction(total, T, MASS)
    k = KJ_PER_MOL_PER_K
    print(f"\n{int(total[:, 0].sum())} molecule samples in {R} chains, T = {T} K")
    print(f"<F^2>           = {ms['f2_pooled']:.6e} +- {ms['f2_err']:.1e} (K/A)^2")
    print(f"<tau^2>         = {ms['tau2_pooled']:.6e} +- {ms['tau2_err']:.1e} K^2")
    print(f"<tau' I^-1 tau> = {ms['t_pooled']:.6e} +- {ms['t_err']:.1e} K^2 / (amu A^2)")
    print(f"dA (Wigner-Kirkwood, first order) = {qc['dA']:.3f} +- {qc['err']:.3f} K per molecule "
          f"= {qc['dA'] * k:.4f} kJ/mol  (translational {qc['translational']:.3f} K, rotational {qc['rotational']:.3f} K)")


if __name__ == "__main__":
    main()
