#!/usr/bin/env python3
"""Hydration free energies at infinite dilution by Widom insertion of FOREIGN solutes into SPC/E
water: R NVT chains as examples/nvt_spce.py runs them, and after every block M insertions per
replica of united-atom methane and of the monoethanolamine (11 sites) of the reference's mixture
deck (tests/golden/decks: mea.pdb + topol.top), as test particles (mmc_batch_widom_solute; the
chains are not disturbed).

    python3 examples/hydration_spce.py [--replicas 256] [--blocks 8] [--sweeps 10] [--insert 256]

Prints mu_ex = -T ln <exp(-dU / T)> of each solute over the run, with its error over the replicas
(every replica is an independent chain with its own sum), in the reference's definition (dU = the
change of its potential(..., "ewald")) and, for the charged solute, minus the intramolecular Ewald
term an inserted molecule brings along (observables.ewald_intra_energy).  The Henry-law volatility
follows as k_H = rho k_B T exp(mu_ex / T).  The numbers are unmeasured until someone runs this: no
assertion on any value.  MEA's LJ rows are its deck parameters mixed against SPC/E by the reference's
rules (structs.Tables).  Needs an MI355X.
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
DECKS = os.path.join(ROOT, "tests", "golden", "decks")


def make_solutes(a):
    """Methane (OPLS united atom: 147.9 K, 3.73 A) and the deck's MEA against the batch's slots."""
    st = np.asarray(a["atype"][:3]) - 1
    e_w, s_w = np.diag(a["eps"])[st], np.diag(a["sig"])[st]

    def rows(eps_site, sig_site):
        eps_site, sig_site = np.asarray(eps_site, dtype=float), np.asarray(sig_site, dtype=float)
        return np.sqrt(eps_site[:, None] * e_w[None, :]), (sig_site[:, None] + s_w[None, :]) / 2

    methane = structs.Solute("methane", np.zeros((1, 3)), [0.0], *rows([147.9], [3.73]))
    top = mio.ReadTopFile(os.path.join(DECKS, "topol.top"), substitutions={"SOLNUMBER": 1})
    m = mio.system_from_decks(mio.ReadPDB(os.path.join(DECKS, "mea.pdb")), top)
    types = [top["atomtypes"][t - 1] for t in m["atype"]]
    mea = structs.Solute("mea", m["coords"] - m["com"][0], m["charge"],
                         *rows([t["epsilon"] / mio.R_GAS for t in types], [t["sigma"] * 10.0 for t in types]))
    return [methane, mea]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--sweeps", type=int, default=10, help="sweeps (N_mol trial moves) per block")
    ap.add_argument("--insert", type=int, default=256, help="insertions per replica and solute after each block")
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
    solutes = make_solutes(a)
    sums = {s.name: (np.zeros(R), np.zeros(R, dtype=np.int64)) for s in solutes}
    for blk in range(1, args.blocks + 1):
        b.run_chains(chains, args.sweeps * n_mol, T, seed=11234 + 1000 * blk, adjust=True, n_threads=2)
        for s in solutes:
            b.widom_solute(s, args.insert, T, seed=99, draw0=blk * args.insert,
                           boltz_sum=sums[s.name][0], n_overlap=sums[s.name][1])
        print(f"block {blk:3d}: <E>/N = {chains['energy'].mean() / n_mol:9.2f} K")
    n_rep = args.blocks * args.insert
    k = KJ_PER_MOL_PER_K
    for s in solutes:
        bs, no = sums[s.name]
        mu = float(observables.widom_mu_ex(bs.sum(), R * n_rep, T))
        with np.errstate(divide="ignore"):
            mu_r = observables.widom_mu_ex(bs, n_rep, T)        # one estimate per replica
        ok = np.isfinite(mu_r)
        err = float(np.std(mu_r[ok], ddof=1) / np.sqrt(ok.sum())) if ok.sum() > 1 else float("nan")
        intra = observables.ewald_intra_energy(s.offsets, s.charge, b.kappa, b.factor) if s.n_sites > 1 else 0.0
        print(f"{s.name}: {s.n_sites} sites, {R * n_rep} insertions, {int(no.sum())} of weight 0, "
              f"{int(R - ok.sum())} replicas without a finite estimate")
        print(f"  mu_ex, reference definition: {mu:.2f} +- {err:.2f} K = {mu * k:.3f} +- {err * k:.3f} kJ/mol")
        if s.n_sites > 1:
            print(f"  mu_ex, physical (minus the intramolecular Ewald term {intra:.2f} K): {mu - intra:.2f} K = "
                  f"{(mu - intra) * k:.3f} kJ/mol")
    b.close()


if __name__ == "__main__":
    main()
