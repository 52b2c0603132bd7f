#!/usr/bin/env python3
"""The distribution p(u) of pair interaction energies of SPC/E water and what follows from it: the
hydrogen-bond peak near -5.5 kcal/mol, the minimum between it and the peak of distant pairs, the
number of hydrogen bonds per molecule by the energetic criterion u < -2.25 kcal/mol (Jorgensen,
Chandrasekhar, Madura, Impey and Klein, J. Chem. Phys. 79, 926, 1983) beside the geometric count of
mmc_batch_local_order, and the potential energy per molecule by distance, E(R).  R NVT chains as
examples/nvt_spce.py runs them (Loop(), Ewald/main.jl:460-696); after equilibration the chains run in
blocks of sweeps and between the blocks mmc_batch_pair_energy and mmc_batch_local_order are taken,
per replica.  The chains are not disturbed.

    python3 examples/pair_energy_spce.py [--replicas 64] [--equil 20] [--blocks 20] [--sweeps 1] [--bins 50]

Prints p(u) on a coarse grid with the standard error over chains, the position of the hydrogen-bond
peak and of the minimum (or that the sample shows only a shoulder), the bonds per molecule from energy and from geometry with their
distributions, and <u_C>(r), <u_LJ>(r) and E(R) on a few radii.  No assertion on the values: runs this
short are far from converged.  Needs an MI355X.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import io as mio, observables, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402

KCAL = 503.22                       # K per kcal/mol
U_LO, U_HI, E_BINS = -4000.0, 2000.0, 120
U_HB = -2.25 * KCAL                 # -1132.2 K


def mean_err(x):
    """Mean and standard error over the leading (chain) axis."""
    x = np.asarray(x, dtype=float)
    err = x.std(0, ddof=1) / np.sqrt(x.shape[0]) if x.shape[0] > 1 else np.full(x.shape[1:], np.nan)
    return x.mean(0), err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=64)
    ap.add_argument("--equil", type=int, default=20, help="sweeps before sampling")
    ap.add_argument("--blocks", type=int, default=20, help="sampled frames")
    ap.add_argument("--sweeps", type=int, default=1, help="sweeps per block")
    ap.add_argument("--bins", type=int, default=50)
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
    rows = np.zeros((R, 3, args.bins + 2), dtype=np.int64)
    uhist = np.zeros((R, E_BINS + 2), dtype=np.uint64)
    nhb = np.zeros((R, 9), dtype=np.uint64)
    geo = np.zeros((R, 3, 9), dtype=np.uint64)
    flagged = 0
    for s in range(args.blocks):
        b.run_chains(chains, args.sweeps * n_mol, T, seed=20000 + s, adjust=False, n_threads=2)
        pe = b.pair_energy(args.bins, 0.0, E_BINS, U_LO, U_HI, U_HB, per_replica=True)   # bins of (L / 2) / bins
        rows += pe.rows
        uhist += pe.uhist
        nhb += pe.nhb
        flagged += int(pe.flagged.sum())
        geo += b.local_order(per_replica=True)["hb_hist"]
    b.close()

    print(f"{R} chains, {args.blocks} frames {args.sweeps} sweep(s) apart, {n_mol} molecules, T = {T} K, L = {box} A; "
          f"pairs within L / 2, {flagged} flagged")
    centres, p = observables.pair_energy_distribution(uhist, n_mol, U_LO, U_HI, args.blocks)
    pm, pe_ = mean_err(p)
    print("   u / (kcal/mol)   p(u) / (pairs per molecule per kcal/mol)")
    for k in range(2, E_BINS, 6):
        print(f"{centres[k] / KCAL:12.2f}      {pm[k] * KCAL:9.4f} +- {pe_[k] * KCAL:7.4f}")
    # the hydrogen-bond peak: a local maximum of p(u) (five-bin running mean) below -3 kcal/mol with a
    # minimum at least a tenth lower between it and the main peak; a short run, or a model with a weak
    # peak, shows a shoulder there and no minimum
    sm = np.convolve(pm, np.ones(5) / 5.0, mode="same")
    main_peak = int(np.argmax(pm))
    peaks = [k for k in range(3, main_peak - 2)
             if centres[k] < -3.0 * KCAL and sm[k] > 0 and sm[k] >= sm[k - 1] and sm[k] > sm[k + 1]
             and sm[k:main_peak].min() < 0.9 * sm[k]]
    if peaks:
        bonded = max(peaks, key=lambda k: sm[k])
        lo = bonded + int(np.argmin(sm[bonded:main_peak]))
        print(f"hydrogen-bond peak at {centres[bonded] / KCAL:.2f} kcal/mol, minimum at {centres[lo] / KCAL:.2f} kcal/mol "
              f"(Jorgensen's criterion: {U_HB / KCAL:.2f}), main peak at {centres[main_peak] / KCAL:.2f} kcal/mol")
    else:
        print(f"p(u) has a shoulder but no separate hydrogen-bond peak below -3 kcal/mol in this sample; "
              f"main peak at {centres[main_peak] / KCAL:.2f} kcal/mol")

    pn, mean = observables.energetic_hbonds(nhb)
    m_e, e_e = mean_err(mean)
    gh = geo[:, 2].astype(float)                       # total = donated + accepted, molecules over n = 0..8
    m_g, e_g = mean_err((gh * np.arange(9)).sum(-1) / gh.sum(-1))
    print(f"hydrogen bonds per molecule: {m_e:.3f} +- {e_e:.3f} from energy (u < {U_HB:.1f} K), "
          f"{m_g:.3f} +- {e_g:.3f} from geometry (r_OO < 3.5 A, angle < 30 deg)")
    print("   n      energy   geometry   (fraction of molecules with n bonds; the last row is 8 or more)")
    pg = mean_err(gh / gh.sum(-1, keepdims=True))[0]
    for k in range(9):
        print(f"{k:4d}   {mean_err(pn)[0][k]:9.4f}  {pg[k]:9.4f}")

    dr = box / 2 / args.bins
    cm, ce = mean_err(observables.pair_energy_profile(rows, n_mol, args.blocks)[2])
    ucm, uljm, _ = observables.pair_energy_profile(rows.sum(0), n_mol, args.blocks * R)   # all chains' pairs together
    print("   R / A    <u_C>(r) / K   <u_LJ>(r) / K   E(R) / (kcal/mol per molecule)")
    for k in range(max(args.bins // 12, 1), args.bins + 1, max(args.bins // 12, 1)):
        print(f"{k * dr:8.3f}   {ucm[k]:12.2f}   {uljm[k]:12.2f}   {cm[k] / KCAL:10.4f} +- {ce[k] / KCAL:6.4f}")
    print(f"pair energy per molecule within L / 2: {cm[-1] / KCAL:.3f} +- {ce[-1] / KCAL:.3f} kcal/mol "
          "(bare Coulomb and LJ, molecule-based cutoff: not the Ewald energy)")


if __name__ == "__main__":
    main()
