#!/usr/bin/env python3
"""First-shell structure of SPC/E water from R NVT chains as examples/nvt_spce.py runs them (Loop(),
Ewald/main.jl:460-696): after equilibration, once per sweep, the hydrogen bonds per molecule
(geometric criterion: O-O closer than 3.5 A, H-O...O angle within 30 degrees) and the tetrahedral
order parameter q of Errington and Debenedetti of every molecule of every replica
(mmc_batch_local_order, per replica).  The chains are not disturbed.

    python3 examples/local_order_spce.py [--replicas 64] [--equil 20] [--sweeps 40] [--bins 400]

Prints <n_HB> (donated, accepted, total) and <q> with the standard error over chains (each chain's
own histogram gives its own mean), the share of molecules by number of bonds, and the most likely q.
No assertion on the values.  Needs an MI355X.
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
    ap.add_argument("--sweeps", type=int, default=40, help="sampled sweeps")
    ap.add_argument("--bins", type=int, default=400)
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
    hb_hist = np.zeros((R, 3, 9), dtype=np.uint64)
    q_hist = np.zeros((R, args.bins), dtype=np.uint64)
    q_sum = np.zeros((R, 2))
    for s in range(args.sweeps):
        b.run_chains(chains, n_mol, T, seed=20000 + s, adjust=False, n_threads=2)
        out = b.local_order(args.bins, per_replica=True)
        hb_hist += out["hb_hist"]
        q_hist += out["q_hist"]
        q_sum += out["q_sum"]
    b.close()

    def with_error(x):                                   # mean over chains and its standard error
        return x.mean(0), (x.std(0, ddof=1) / np.sqrt(R) if R > 1 else np.full(x.shape[1:], np.nan))

    print(f"{R} chains, {args.sweeps} sampled sweeps of {n_mol} molecules, T = {T} K, L = {box} A")
    n_hb, n_err = with_error(observables.hbonds_per_molecule(hb_hist))            # [R, 3]
    for k, name in enumerate(("donated", "accepted", "total")):
        print(f"<n_HB> {name:8s}: {n_hb[k]:.3f} +- {n_err[k]:.3f}")
    share = hb_hist[:, 2].sum(0) / hb_hist[:, 2].sum()
    print("molecules with n = 0..8 bonds: " + " ".join(f"{x:.3f}" for x in share))
    q, q_err = with_error(observables.tetrahedral_mean(q_sum)[:, None])
    print(f"<q>: {q[0]:.4f} +- {q_err[0]:.4f}")
    centres, dens = observables.normalize_q_hist(q_hist.sum(0))
    print(f"P(q) peaks at q = {centres[np.argmax(dens)]:.3f} (density {dens.max():.2f})")


if __name__ == "__main__":
    main()
