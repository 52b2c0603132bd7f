#!/usr/bin/env python3
"""Hydration shells of a solute held fixed in SPC/E water: R NVT chains that feel the solute as
molecule N + 1 (mmc_batch_set_solute), for united-atom methane and for a sodium-like cation, each in
its own batch of 750 waters (NIST configuration 4).

    python3 examples/hydration_shell_spce.py [--replicas 64] [--blocks 10] [--sweeps 4] [--equil 10]

The solute is set in the largest cavity of the starting configuration; after `--equil` sweeps every
block of `--sweeps` sweeps ends with one sample of the solute-oxygen histogram of every replica
(mmc_batch_rdf_solute) and of the water-solute pair energy (mmc_batch_solute_energy).  Prints
g_CO(r) (g_NaO(r)) around its first peak, the first-shell coordination number -- the running integral
at the first minimum of g beyond that peak -- and the solvation energy <u_sw>, each with its error
over the replicas (every replica is an independent chain).  A charged solute gets no neutralising
background and no intramolecular term, as the reference's total energy has neither.  The numbers are
unmeasured until someone runs this: no assertion on any value.  Needs an MI355X.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import io as mio, observables, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402

NUMBINS, R_MAX = 150, 7.5


def make_solutes(a):
    """Methane (OPLS united atom: 147.9 K, 3.73 A) and a cation (q = +1, 65.4 K, 2.35 A) against the
    batch's three atom slots, mixed by the reference's rules (structs.Tables)."""
    st = np.asarray(a["atype"][:3]) - 1
    e_w, s_w = np.diag(a["eps"])[st], np.diag(a["sig"])[st]

    def one(name, q, eps, sig):
        return structs.Solute(name, np.zeros((1, 3)), [q], np.sqrt(eps * e_w)[None, :], ((sig + s_w) / 2)[None, :])
    return [one("methane", 0.0, 147.9, 3.73), one("cation", 1.0, 65.4, 2.35)]


def cavity(a, n_try=4000, seed=1):
    """The candidate point (of n_try uniform ones) farthest from every atom, by the minimum image."""
    box = float(a["box"])
    pts = np.random.default_rng(seed).random((n_try, 3)) * box
    d = pts[:, None, :] - np.asarray(a["coords"])[None, :, :]
    d -= box * np.round(d / box)
    m = np.sqrt((d * d).sum(2)).min(1)
    return pts[int(m.argmax())]


def mean_err(x):
    x = np.asarray(x, dtype=float)
    return float(x.mean()), float(x.std(ddof=1) / np.sqrt(x.shape[0])) if x.shape[0] > 1 else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--sweeps", type=int, default=4, help="sweeps (N_mol trial moves) per block")
    ap.add_argument("--equil", type=int, default=10, help="sweeps before the first sample")
    ap.add_argument("--temperature", type=float, default=298.15)
    args = ap.parse_args()
    T, R = args.temperature, args.replicas

    a = mio.load_nist_fixture(4, "unwrapped")
    n_mol, box, r_cut = a["com"].shape[0], a["box"], 10.0
    dr = R_MAX / NUMBINS
    c = cavity(a)
    for sol in make_solutes(a):
        b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, 5.6 / box,
                  structs.factor, r_cut, r_cut)
        b.set_option("device_moves", 1)
        b.set_solute(sol, np.vstack([c + sol.offsets, c]))
        tot = b.potential_ewald()                               # (also builds S(k) of the N + 1 system)
        chains = b.new_chains([t["energy"] for t in tot], [t["virial"] for t in tot], dr_max=0.316555789, dphi_max=0.05)
        b.run_chains(chains, args.equil * n_mol, T, seed=4321, adjust=True, n_threads=2)
        hist = np.zeros((R, 2, 3, NUMBINS), dtype=np.uint64)
        u_sw = np.zeros(R)
        for blk in range(1, args.blocks + 1):
            b.run_chains(chains, args.sweeps * n_mol, T, seed=11234 + 1000 * blk, adjust=True, n_threads=2)
            hist += b.rdf_solute(NUMBINS, R_MAX, per_replica=True)
            u_lj, u_real, _ = b.solute_energy()
            u_sw += u_lj + u_real
        b.close()
        # g(r) from the reference point against the oxygens (slot 0), per replica
        rows = hist[:, 0, 0, :].astype(float)
        r, g = observables.normalize_rdf_solute(rows, n_mol, dr, args.blocks / box ** 3)
        g_mean = g.mean(0)
        k_peak = int(np.argmax(g_mean))
        k_min = k_peak + int(np.argmin(g_mean[k_peak:min(k_peak + int(2.5 / dr), NUMBINS)]))
        n_shell = observables.coordination_number(rows, args.blocks, dr, r_shell=(k_min + 1) * dr)
        print(f"{sol.name} (q = {sol.charge[0]:+.1f}) in {n_mol} SPC/E, {R} replicas x {args.blocks} samples")
        for k in range(max(k_peak - 6, 0), min(k_min + 7, NUMBINS), 2):
            m, e = mean_err(g[:, k])
            print(f"  g_XO({r[k]:5.3f} A) = {m:6.3f} +- {e:5.3f}")
        m, e = mean_err(n_shell)
        print(f"  first peak at {r[k_peak]:.3f} A, first minimum at {r[k_min]:.3f} A, coordination number {m:.2f} +- {e:.2f}")
        m, e = mean_err(u_sw / args.blocks)
        print(f"  <u_sw> = {m:.1f} +- {e:.1f} K = {m * structs.R:.2f} +- {e * structs.R:.2f} kJ/mol")


if __name__ == "__main__":
    main()
