#!/usr/bin/env python3
"""Independent NPT chains of SPC/E water in ONE batch, a box per replica: a density-vs-pressure
scan.  Every replica starts from the NIST SPC/E sample configuration 4 (750 molecules, = Ewald/
coord750.txt) and runs Loop()'s trial moves (Ewald/main.jl:487-644) interleaved with the volume
move of Ewald/volumeChange.jl:59-147 at its own pressure; the volume moves of all replicas are one
batched trial on the device (mmc_batch_run_npt_replicas).

    python3 examples/npt_replicas.py [--pressures-bar 1,1000,4000] [--chains 4] [--blocks 10] [--sweeps 40]

Needs an MI355X (no CPU fallback).  The NIST configuration is at 0.83 g/cm3 and the chains compress
from there; every chain follows the rule and energy model of examples/npt_spce.py, whose one
replica makes the same decisions (tests/test_gpu_npt_replicas.py) and ends at the same density
(about 1.37 g/cm3 after 10 x 40 sweeps at 1 bar, not yet equilibrated).  The chains at one pressure are
independent replicas (streams replica0 + r); <V> and the density are averaged over the volume moves
of the second half of the blocks and over the chains at that pressure.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import io as mio, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402

BAR_IN_K_PER_A3 = 1e5 / 1.380649e-23 * 1e-30      # 1 bar = 7.2430e-3 K / A^3
G_PER_CM3 = 18.01528 / 0.602214076                 # molecules / A^3 -> g / cm^3 of water


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pressures-bar", default="1,1000,4000")
    ap.add_argument("--chains", type=int, default=4, help="chains per pressure")
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--sweeps", type=int, default=40, help="sweeps (N_mol trial moves + 1 volume move) per block")
    ap.add_argument("--temperature", type=float, default=298.15)
    ap.add_argument("--vmax-frac", type=float, default=0.01, help="dV uniform in +- this fraction of V / 2")
    args = ap.parse_args()

    a = mio.load_nist_fixture(4, "unwrapped")
    p_bar = [float(x) for x in args.pressures_bar.split(",")]
    n_p, n_c = len(p_bar), args.chains
    R = n_p * n_c
    n_mol, box, r_cut, alpha = a["com"].shape[0], float(a["box"]), 10.0, 5.6
    pressures = np.repeat(np.array(p_bar) * BAR_IN_K_PER_A3, n_c)   # replica r: pressure r // chains
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, alpha / box,
              structs.factor, r_cut, r_cut)
    b.set_boxes(np.full(R, box), alpha)
    b.recip_long()
    energies = b.potential_ewald(as_array=True)["energy"].copy()
    vmax = args.vmax_frac * box ** 3
    print(f"{R} chains of {n_mol} SPC/E molecules ({n_c} per pressure), L0 = {box:.4f} A, T = {args.temperature} K")
    vsum, nvol = np.zeros(R), np.zeros(R)
    for blk in range(1, args.blocks + 1):
        energies, st, ns = b.run_npt_replicas(args.sweeps, args.temperature, 0.0, vmax, 0.316555789, 0.05,
                                              seed=11234 + blk, energies=energies, alpha=alpha,
                                              pressures=pressures)
        if blk > args.blocks // 2:
            vsum += [x["volume_sum"] for x in ns]
            nvol += [x["vol_attempt"] for x in ns]
        L = np.array([x["box"] for x in ns])
        acc = (st["trans_accept"] + st["rot_accept"]) / max(st["moves"], 1)
        vacc = sum(x["vol_accept"] for x in ns) / max(sum(x["vol_attempt"] for x in ns), 1)
        print(f"Block: {blk:3d}, mean density: {np.mean(n_mol / L ** 3) * G_PER_CM3:6.4f} g/cm3, move ratio: "
              f"{acc:4.2f}, volume ratio: {vacc:4.2f}, us/move: {1e3 * st['wall_ms'] / max(st['moves'], 1):6.2f}, "
              f"ms/batched volume move: {ns[0]['volume_ms'] / max(ns[0]['vol_attempt'], 1):6.2f}")
    check = b.potential_ewald(as_array=True)["energy"]
    print(f"running totals against recomputed: max relative difference "
          f"{np.max(np.abs(energies - check) / np.abs(check)):.2e}")
    print(f"{'P / bar':>10} {'<V> / A^3':>12} {'density / g cm-3':>18}")
    for k, p in enumerate(p_bar):
        sl = slice(k * n_c, (k + 1) * n_c)
        v = vsum[sl].sum() / nvol[sl].sum() if nvol[sl].sum() else float(np.mean(L[sl] ** 3))
        print(f"{p:10.1f} {v:12.1f} {n_mol / v * G_PER_CM3:18.4f}")
    b.close()


if __name__ == "__main__":
    main()
