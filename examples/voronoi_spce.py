#!/usr/bin/env python3
"""Voronoi cells of SPC/E water from R NVT chains as examples/nvt_spce.py runs them (Loop(),
Ewald/main.jl:460-696): after equilibration, once per sweep, the Voronoi cell of every oxygen of every
replica from its O-O neighbours inside r_list (mmc_batch_voronoi, per replica) -- its volume, its
asphericity eta = S^3 / (36 pi V^2), its geometric neighbours.  The chains are not disturbed.

    python3 examples/voronoi_spce.py [--replicas 256] [--equil 20] [--sweeps 40] [--r-list 7.5]

Prints <V>, <V^2> - <V>^2, <eta> and the mean geometric coordination number with the standard error
over chains, the coordination distribution, the mean number of sides of a face, and the fraction of
the cells that were flagged (left out: a cell is certified only when every vertex lies within
r_list / 2, so at low density the largest cells are missing and <V> is biased low by about that
fraction).  No assertion on the values.  Needs an MI355X.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import io as mio, observables, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402

AREA_MIN = 1e-6     # A^2: a face of rounding is not a neighbour


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=256)
    ap.add_argument("--equil", type=int, default=20, help="sweeps before sampling")
    ap.add_argument("--sweeps", type=int, default=40, help="sampled sweeps")
    ap.add_argument("--temperature", type=float, default=298.15)
    ap.add_argument("--r-list", type=float, default=7.5)
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
    acc = None
    for s in range(args.sweeps):
        b.run_chains(chains, n_mol, T, seed=20000 + s, adjust=False, n_threads=2)
        out = b.voronoi(r_list=args.r_list, area_min=AREA_MIN, per_replica=True)
        if acc is None:
            acc = out
        else:
            for k in acc:
                acc[k] += out[k]
    b.close()

    def with_error(x):                                   # mean over chains and its standard error
        return x.mean(0), (x.std(0, ddof=1) / np.sqrt(R) if R > 1 else np.nan)

    cells = R * args.sweeps * n_mol
    print(f"{R} chains, {args.sweeps} sampled sweeps of {n_mol} molecules, T = {T} K, L = {box} A, r_list = {args.r_list} A")
    cap, opened, poly = (int(v) for v in acc["flagged"].sum(0))
    print(f"flagged: {(cap + opened + poly) / cells:.4f} of {cells} cells (more than 64 neighbours in range: {cap}; "
          f"a vertex beyond r_list / 2: {opened}; a face beyond 16 vertices: {poly})")
    v, eta, faces = observables.voronoi_means(acc["sums"])                                   # [R] each
    for name, x, unit in (("<V>", v, " A^3"), ("<V^2> - <V>^2", observables.volume_fluctuation(acc["sums"]), " A^6"),
                          ("<eta>", eta, ""), ("<faces>", faces, "")):
        m, err = with_error(x)
        print(f"{name}: {m:.4f} +- {err:.4f}{unit}")
    print(f"L^3 / N = {box ** 3 / n_mol:.4f} A^3")
    n, p, mean = observables.voronoi_coordination(acc["face_hist"].sum(0))
    print("geometric coordination: " + "  ".join(f"{k}: {p[k]:.4f}" for k in n if p[k] >= 5e-5))
    k, pk, sides = observables.face_side_fractions(acc["side_hist"].sum(0))
    print(f"sides of a face: {sides:.4f} on average (6 - 12 / <faces> = {6.0 - 12.0 / mean:.4f}); "
          + "  ".join(f"{j}: {pk[j]:.4f}" for j in k if pk[j] >= 5e-5))
    x, pe, beyond = observables.asphericity_distribution(acc["eta_hist"].sum(0), 3.0)
    print(f"P(eta) peaks at {x[np.argmax(pe)]:.3f} (2.25 in ice Ih; beyond 3: {beyond:.2e})")


if __name__ == "__main__":
    main()
