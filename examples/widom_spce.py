#!/usr/bin/env python3
"""Excess chemical potential of SPC/E water by Widom test-particle insertion: R NVT chains as
examples/nvt_spce.py runs them (Loop(), Ewald/main.jl:460-696), and after every block M insertions
of a rigid SPC/E molecule per replica (mmc_batch_widom; the chains are not disturbed).

    python3 examples/widom_spce.py [--replicas 256] [--blocks 8] [--sweeps 10] [--insert 64]

Prints mu_ex = -T ln <exp(-dU / T)> per block and over the run with its block error, in two
definitions: the reference's (dU = the change of its potential(..., "ewald"), which leaves out the
intramolecular Ewald term -- quirk Q10) and the physical one (minus that term,
observables.ewald_intra_energy).  No assertion on the value.  Needs an MI355X.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--sweeps", type=int, default=10, help="sweeps (N_mol trial moves) per block")
    ap.add_argument("--insert", type=int, default=64, help="insertions per replica after each block")
    ap.add_argument("--temperature", type=float, default=298.15)
    args = ap.parse_args()
    T = args.temperature

    a = mio.load_nist_fixture(4, "unwrapped")
    n_mol, box, r_cut = a["com"].shape[0], a["box"], 10.0
    b = Batch(args.replicas, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box,
              5.6 / box, structs.factor, r_cut, r_cut)
    b.set_option("device_moves", 1)
    tot = b.potential_ewald()                                   # main.jl:408 (also builds S(k))
    chains = b.new_chains([t["energy"] for t in tot], [t["virial"] for t in tot],
                          dr_max=0.316555789, dphi_max=0.05)
    intra = observables.ewald_intra_energy(b.widom_offsets, b.charge3, b.kappa, b.factor)
    total_w, total_n, block_mu = 0.0, 0, []
    for blk in range(1, args.blocks + 1):
        b.run_chains(chains, args.sweeps * n_mol, T, seed=11234 + 1000 * blk, adjust=True, n_threads=2)
        bs, no = b.widom(args.insert, T, seed=99, draw0=blk * args.insert)
        n = args.replicas * args.insert
        mu = float(observables.widom_mu_ex(bs.sum(), n, T))
        block_mu.append(mu)
        total_w += bs.sum()
        total_n += n
        print(f"block {blk:3d}: <E>/N = {chains['energy'].mean() / n_mol:9.2f} K, "
              f"mu_ex(reference) = {mu:9.2f} K, overlaps {int(no.sum())} of {n}")
    mu = float(observables.widom_mu_ex(total_w, total_n, T))
    err = float(np.std(block_mu, ddof=1) / np.sqrt(len(block_mu))) if len(block_mu) > 1 else float("nan")
    k = KJ_PER_MOL_PER_K
    print(f"{total_n} insertions into {args.replicas} chains, T = {T} K; intramolecular Ewald term "
          f"{intra:.2f} K ({intra * k:.3f} kJ/mol)")
    print(f"mu_ex, reference definition: {mu:.2f} +- {err:.2f} K = {mu * k:.3f} +- {err * k:.3f} kJ/mol")
    print(f"mu_ex, physical:             {mu - intra:.2f} +- {err:.2f} K = {(mu - intra) * k:.3f} +- "
          f"{err * k:.3f} kJ/mol")
    b.close()


if __name__ == "__main__":
    main()
