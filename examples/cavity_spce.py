#!/usr/bin/env python3
"""Cavity statistics of SPC/E water from R NVT chains as examples/nvt_spce.py runs them (Loop(),
Ewald/main.jl:460-696): after equilibration, once per sweep, the number of oxygens within R of
random points of every replica and the distance of the nearest oxygen (mmc_batch_cavity).  The
chains are not disturbed.

    python3 examples/cavity_spce.py [--replicas 64] [--equil 20] [--sweeps 40] [--probes 750]

Prints the occupancy distribution p_n of a sphere of radius 3.3 A (the exclusion radius of a
methane-sized solute about the water oxygens), and, from the nearest-oxygen histogram, the hard-sphere
excess chemical potential mu_ex(R) = -T ln p_0(R) on a grid of radii -- beside it the p_0 that the
two-moment information-theory model (Hummer et al., PNAS 93, 8951, 1996) predicts from <n> and
<dn^2> alone and the p_0 counted directly.  No assertion on the values.  Needs an MI355X.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import io as mio, observables as obs, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402

NN_BINS, NN_MAX = 400, 5.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=64)
    ap.add_argument("--equil", type=int, default=20, help="sweeps before sampling")
    ap.add_argument("--sweeps", type=int, default=40, help="sampled sweeps")
    ap.add_argument("--probes", type=int, default=750, help="probe points per replica and sweep")
    ap.add_argument("--temperature", type=float, default=298.15)
    args = ap.parse_args()
    T, R, P = args.temperature, args.replicas, args.probes

    a = mio.load_nist_fixture(4, "unwrapped")
    n_mol, box, r_cut = a["com"].shape[0], a["box"], 10.0
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box,
              5.6 / box, structs.factor, r_cut, r_cut)
    b.set_option("device_moves", 1)
    tot = b.potential_ewald()
    chains = b.new_chains([t["energy"] for t in tot], [t["virial"] for t in tot],
                          dr_max=0.316555789, dphi_max=0.05)
    b.run_chains(chains, args.equil * n_mol, T, seed=11234, adjust=True, n_threads=2)
    dr = NN_MAX / NN_BINS
    ms = [80 * k for k in range(1, 5)] + [264]               # 1, 2, 3, 4 and 3.3 A as edges of the grid
    ms.sort()
    radii = [m * dr for m in ms]
    acc = None
    for s in range(args.sweeps):
        b.run_chains(chains, n_mol, T, seed=20000 + s, adjust=False, n_threads=2)
        out = b.cavity(P, seed=777, draw0=s * P, radii=radii, n_cap=40, nn_bins=NN_BINS, nn_max=NN_MAX)
        acc = out if acc is None else {k: acc[k] + out[k] for k in out}
    b.close()

    n_total = R * P * args.sweeps
    print(f"{R} chains, {args.sweeps} sampled sweeps of {n_mol} molecules, {n_total} probe spheres, T = {T} K, L = {box} A")
    k33 = ms.index(264)
    p_n = obs.occupancy_probabilities(acc["occ_hist"], allow_overflow=True)
    print(f"p_n at R = {radii[k33]:.2f} A, n = 0..12: " + " ".join(f"{x:.2e}" for x in p_n[k33, :13]))
    mean, var = obs.occupancy_moments(acc["occ_mom"], n_total)
    edges, p0 = obs.cavity_size_distribution(acc["nn_hist"], NN_MAX)
    mu = obs.cavity_mu_ex(p0, T)
    print("    R / A      <n>   <dn^2>   p0 direct   p0 inf. theory   mu_ex(direct) / K")
    for k, m in enumerate(ms):
        try:
            p0_it = obs.information_theory_pn(mean[k], var[k], 40)[0]
        except ValueError:
            p0_it = float("nan")
        print(f"  {edges[m]:7.3f}  {mean[k]:7.3f}  {var[k]:7.3f}  {p0[m]:10.3e}  {p0_it:15.3e}  {mu[m]:18.1f}")
    seen = np.flatnonzero(acc["nn_hist"])
    print(f"largest cavity seen: no oxygen within {edges[seen[-1]]:.3f} A of a point")


if __name__ == "__main__":
    main()
