#!/usr/bin/env python3
"""The methane-methane potential of mean force in SPC/E water at infinite dilution, by Widom
insertion of solute PAIRS: R NVT chains as examples/nvt_spce.py runs them, and after every block M
insertions per replica of two united-atom methanes, the second at K separations from the first
along one random ray per insertion (mmc_batch_widom_pair; the chains are not disturbed).

    python3 examples/pmf_methane_spce.py [--replicas 256] [--blocks 8] [--sweeps 10] [--insert 256]

By the potential distribution theorem
    g(d) = <exp(-dU_AB(d) / T)> / (<exp(-dU_A / T)> <exp(-dU_B / T)>),    w(d) = -T ln g(d),
all three averages over the same insertions (observables.pair_pmf).  Prints w(d) on the grid of
separations -- the contact minimum near 3.9 A, the desolvation barrier and the solvent-separated
minimum near 7 A are what to look for -- with its error over the replicas (every replica is an
independent chain with its own sums), and the direct methane-methane LJ energy beside it.  The
numbers are unmeasured until someone runs this: no assertion on any value.  Needs an MI355X.
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
EPS, SIG = 147.9, 3.73        # OPLS united-atom methane (K, A)


def methane_pair(a):
    st = np.asarray(a["atype"][:3]) - 1
    e_w, s_w = np.diag(a["eps"])[st], np.diag(a["sig"])[st]
    m = structs.Solute("methane", np.zeros((1, 3)), [0.0], np.sqrt(EPS * e_w)[None, :], ((SIG + s_w) / 2)[None, :])
    return structs.SolutePair(m, m, [[EPS]], [[SIG]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--sweeps", type=int, default=10, help="sweeps (N_mol trial moves) per block")
    ap.add_argument("--insert", type=int, default=256, help="pair insertions per replica after each block")
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
    pair = methane_pair(a)
    d = np.arange(3.4, 10.01, 0.3)                              # 23 separations, all below box / 2
    sums = None
    for blk in range(1, args.blocks + 1):
        b.run_chains(chains, args.sweeps * n_mol, T, seed=11234 + 1000 * blk, adjust=True, n_threads=2)
        sums = b.widom_pair(pair, d, args.insert, T, seed=99, draw0=blk * args.insert, sums=sums)
        print(f"block {blk:3d}: <E>/N = {chains['energy'].mean() / n_mol:9.2f} K")
    n_rep = args.blocks * args.insert
    pmf = observables.pair_pmf(sums["boltz_ab"], sums["boltz_a"], sums["boltz_b"], n_rep, T)
    mu = float(observables.widom_mu_ex(sums["boltz_a"].sum(), R * n_rep, T))
    k = KJ_PER_MOL_PER_K
    print(f"{R * n_rep} pair insertions per separation; mu_ex(methane) = {mu:.1f} K = {mu * k:.2f} kJ/mol")
    print("   d / A      g(d)    w(d) / K   +- (replicas)   w / kJ/mol   u_LJ(d) / K")
    for i, dk in enumerate(d):
        s6 = (SIG / dk) ** 6
        print(f"  {dk:6.2f}  {pmf['g'][i]:8.3f}  {pmf['w'][i]:10.1f}  {pmf['w_err'][i]:12.1f}  "
              f"{pmf['w'][i] * k:10.3f}  {4 * EPS * (s6 * s6 - s6):11.1f}")
    b.close()


if __name__ == "__main__":
    main()
