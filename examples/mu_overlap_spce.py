#!/usr/bin/env python3
"""Excess chemical potential of SPC/E water from BOTH test-particle distributions: R NVT chains as
examples/nvt_spce.py runs them (Loop(), Ewald/main.jl:460-696), and after every block M random
insertions per replica (mmc_batch_widom, the energies through du_out) and the deletion energies of
K randomly chosen molecules per replica (mmc_batch_deletion, histogrammed on the device).  Neither
call disturbs the chains.

    python3 examples/mu_overlap_spce.py [--replicas 256] [--blocks 8] [--sweeps 10] [--insert 64] [--delete 64]

Prints, side by side, mu_ex by one-sided Widom insertion (-T ln <exp(-dU / T)>), by inverse Widom
(+T ln <exp(+dU / T)> over the deletions), by Bennett's acceptance ratio with its standard error
(observables.bennett_mu_ex on the two histograms), and the overlapping-distribution curve
T (ln g - ln f) + u, which is flat at mu_ex where both histograms are populated
(observables.overlap_curves).  All in the reference's definition of the energy (its
potential(..., "ewald") leaves out the intramolecular Ewald term, quirk Q10); the physical value is
that minus observables.ewald_intra_energy, printed at the end.  Insertions that overlap count as
insertions of energy u_hi.  No assertion on any value.  Needs an MI355X.
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
BINS = (320, -60000.0, 20000.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--sweeps", type=int, default=10, help="sweeps (N_mol trial moves) per block")
    ap.add_argument("--insert", type=int, default=64, help="insertions per replica after each block")
    ap.add_argument("--delete", type=int, default=64, help="deletion energies per replica after each block")
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
    rng = np.random.default_rng(2024)
    n_bins, u_lo, u_hi = BINS
    hist_ins, hist_del = np.zeros(n_bins + 2, dtype=np.uint64), np.zeros(n_bins + 2, dtype=np.uint64)
    w_ins, n_ins = 0.0, 0
    w_del, n_flag = np.zeros(R), np.zeros(R, dtype=np.int64)
    n_del = 0
    for blk in range(1, args.blocks + 1):
        b.run_chains(chains, args.sweeps * n_mol, T, seed=11234 + 1000 * blk, adjust=True, n_threads=2)
        bs, no, _, du, ovl = b.widom(args.insert, T, seed=99, draw0=blk * args.insert, outputs=True)
        u = (du[..., 0] + du[..., 1]) + du[..., 2]
        hist_ins += observables.energy_bins(np.where(ovl != 0, np.inf, u), n_bins, u_lo, u_hi)
        w_ins += bs.sum()
        n_ins += R * args.insert
        sel = rng.choice(n_mol, size=args.delete, replace=False)
        res = b.deletion(T, sel=sel, bins=BINS, boltz_sum=w_del, n_flagged=n_flag)
        hist_del += res["hist"]
        n_del += R * args.delete
        print(f"block {blk:3d}: <E>/N = {chains['energy'].mean() / n_mol:9.2f} K, insertions {n_ins}, "
              f"deletions {n_del} (flagged {int(n_flag.sum())}), mean binding energy "
              f"{res['esum'][:, :3].sum() / res['esum'][:, 3].sum():10.2f} K")
    b_intra = observables.ewald_intra_energy(b.widom_offsets, b.charge3, b.kappa, b.factor)
    b.close()

    k = KJ_PER_MOL_PER_K
    mu_w = float(observables.widom_mu_ex(w_ins, n_ins, T))
    mu_i = float(T * np.log(w_del.sum() / (n_del - n_flag.sum())))
    centres, ln_f, ln_g, const = observables.overlap_curves(hist_ins, hist_del, n_bins, u_lo, u_hi, T)
    # BAR from the histograms: bin centres with their counts; what fell above the grid (overlapping
    # insertions among it) enters at u_hi, what fell below at u_lo
    u_all = np.concatenate([[u_lo], centres, [u_hi]])
    mu_b, err_b = observables.bennett_mu_ex(u_all, u_all, T, w_ins=hist_ins, w_del=hist_del)
    print(f"\n{n_ins} insertions and {n_del} deletions in {R} chains, T = {T} K")
    print(f"mu_ex, Widom insertion:   {mu_w:10.2f} K = {mu_w * k:8.3f} kJ/mol")
    print(f"mu_ex, inverse Widom:     {mu_i:10.2f} K = {mu_i * k:8.3f} kJ/mol")
    print(f"mu_ex, BAR:               {mu_b:10.2f} +- {err_b:.2f} K = {mu_b * k:8.3f} +- {err_b * k:.3f} kJ/mol")
    print(f"(reference definition; physical = reference - the intramolecular Ewald term of "
          f"{b_intra:.2f} K: BAR {mu_b - b_intra:.2f} K = {(mu_b - b_intra) * k:.3f} kJ/mol)")
    print("\noverlapping distributions (bins with at least 20 counts on both sides):")
    print("      u / K      ln f      ln g   T (ln g - ln f) + u / K")
    for j in range(n_bins):
        if hist_ins[j + 1] >= 20 and hist_del[j + 1] >= 20:
            print(f"{centres[j]:11.1f} {ln_f[j]:9.3f} {ln_g[j]:9.3f} {T * const[j]:12.2f}")


if __name__ == "__main__":
    main()
