#!/usr/bin/env python3
"""Order between the first and second shell of SPC/E water from R NVT chains as examples/nvt_spce.py
runs them (Loop(), Ewald/main.jl:460-696): after equilibration, once per sweep, every molecule's
sorted O-O neighbour list inside 6 A and from it the fifth-neighbour distance d5, the local structure
index (r_lsi = 3.7 A), Russo and Tanaka's zeta (bonds: O-O closer than 3.5 A, H-O...O within 30
degrees) and the O-O-O angles between neighbours inside 3.3 A, of every replica
(mmc_batch_shell_order, per replica).  The chains are not disturbed.

    python3 examples/shell_order_spce.py [--replicas 256] [--equil 20] [--sweeps 40]

Prints <d5>, <I> and <zeta> with the standard error over chains, the two populations of the zeta
histogram (the shares below and above the minimum between its two highest maxima, if it has two, and
each side's mean), and the peak of the O-O-O angle distribution.  No assertion on the values.  Needs
an MI355X.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import io as mio, observables, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402

R_LIST, ZETA_LO, ZETA_HI, LSI_MAX = 6.0, -1.5, 2.5, 0.4


def two_populations(x, p):
    """(split, share below, mean below, mean above) of a density p(x) at the minimum between its two
    highest local maxima (smoothed over five bins); None if it has one maximum only."""
    s = np.convolve(p, np.ones(5) / 5.0, mode="same")
    peaks = [k for k in range(1, len(s) - 1) if s[k] > s[k - 1] and s[k] >= s[k + 1] and s[k] > 0.05 * s.max()]
    if len(peaks) < 2:
        return None
    lo, hi = sorted(sorted(peaks, key=lambda k: -s[k])[:2])
    cut = lo + int(np.argmin(s[lo:hi + 1]))
    w = p / p.sum()
    below = w[:cut].sum()
    return x[cut], below, (w[:cut] * x[:cut]).sum() / below, (w[cut:] * x[cut:]).sum() / (1.0 - below)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=256)
    ap.add_argument("--equil", type=int, default=20, help="sweeps before sampling")
    ap.add_argument("--sweeps", type=int, default=40, help="sampled sweeps")
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
    acc = None
    for s in range(args.sweeps):
        b.run_chains(chains, n_mol, T, seed=20000 + s, adjust=False, n_threads=2)
        out = b.shell_order(r_list=R_LIST, lsi_max=LSI_MAX, zeta_lo=ZETA_LO, zeta_hi=ZETA_HI, per_replica=True)
        if acc is None:
            acc = out
        else:
            for k in acc:
                acc[k] += out[k]
    b.close()

    def with_error(x):                                   # mean over chains and its standard error
        return x.mean(0), (x.std(0, ddof=1) / np.sqrt(R) if R > 1 else np.nan)

    print(f"{R} chains, {args.sweeps} sampled sweeps of {n_mol} molecules, T = {T} K, L = {box} A")
    print(f"flagged (more than 64 neighbours inside {R_LIST} A): {int(acc['flagged'].sum())} of {R * args.sweeps * n_mol}")
    r, pk, beyond = observables.neighbour_distance_distributions(acc["rank_hist"], R_LIST)      # [R, 8, bins]
    d5, d5_err = with_error((pk[:, 4] * r).sum(-1) * (r[1] - r[0]))
    print(f"<d5>: {d5:.4f} +- {d5_err:.4f} A (no fifth neighbour inside {R_LIST} A: {beyond[:, 4].mean():.2e})")
    lsi, lsi_err = with_error(observables.lsi_mean(acc["sums"]))
    print(f"<I>: {lsi:.5f} +- {lsi_err:.5f} A^2")
    zeta, zeta_err = with_error(observables.zeta_mean(acc["sums"]))
    print(f"<zeta>: {zeta:.4f} +- {zeta_err:.4f} A")
    x, p, undefined = observables.zeta_distribution(acc["zeta_hist"].sum(0), ZETA_LO, ZETA_HI)
    pops = two_populations(x, p)
    if pops is None:
        print(f"P(zeta): one maximum, at {x[np.argmax(p)]:.3f} A (undefined for {undefined:.2e} of the molecules)")
    else:
        print(f"P(zeta): two populations split at {pops[0]:.3f} A: {pops[1]:.3f} of the molecules below "
              f"(mean {pops[2]:.3f} A), {1.0 - pops[1]:.3f} above (mean {pops[3]:.3f} A)")
    theta, p_theta, mean_cos = observables.ooo_angle_distribution(acc["ang_hist"].sum(0))
    print(f"P(theta_OOO) peaks at {theta[np.argmax(p_theta)]:.1f} degrees; <cos theta> = {mean_cos:.4f}")


if __name__ == "__main__":
    main()
