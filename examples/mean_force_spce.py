#!/usr/bin/env python3
"""What the water does to a solute held fixed in SPC/E water (mmc_batch_solute_forces), two ways, each in
R NVT chains of 750 waters (NIST configuration 4) that feel the solute as molecule N + 1:

  charging   a sodium-like cation set at charges lambda q for a few lambda: <q phi>_lambda, the potential
             at the site, integrated over lambda by the trapezoid -- the charging free energy of the ion
             (with its periodic images and no neutralising background, as the reference's total has none);
  ion pair   a two-site "solute", the cation and a chloride-like anion, at a handful of separations: the
             solvent's mean force along the axis, integrated from the largest separation -- the solvent's
             part of the potential of mean force.  The reference has no intramolecular term, so the direct
             cation-anion interaction (Lennard-Jones and Coulomb, or its Ewald sum) is the caller's to add.

    python3 examples/mean_force_spce.py [--replicas 64] [--blocks 6] [--sweeps 2] [--equil 6]

Every state point: set_solute, recip_long (S(k) of the N + 1 system), `--equil` sweeps, then `--blocks`
blocks of `--sweeps` sweeps, each ending with one sample of solute_forces of every replica.  Errors are
over the replicas (independent chains).  The numbers are unmeasured until someone runs this: no assertion
on any value.  Needs an MI355X.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import io as mio, observables, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402

LAMBDAS = (0.0, 0.25, 0.5, 0.75, 1.0)
SEPARATIONS = (2.6, 3.0, 3.6, 4.4, 5.2, 6.0)
ION = {"cation": (1.0, 65.4, 2.35), "anion": (-1.0, 50.3, 4.40)}   # charge, eps (K), sig (A)


def solute(a, names, charges, offsets):
    """Sites with their own LJ parameters against the batch's three atom slots, mixed by the reference's
    rules (structs.Tables: sqrt(eps_i eps_j), (sig_i + sig_j) / 2)."""
    st = np.asarray(a["atype"][:3]) - 1
    e_w, s_w = np.diag(a["eps"])[st], np.diag(a["sig"])[st]
    eps = np.array([np.sqrt(ION[n][1] * e_w) for n in names])
    sig = np.array([(ION[n][2] + s_w) / 2 for n in names])
    return structs.Solute("+".join(names), offsets, charges, eps, sig)


def cavity(a, offsets, n_try=4000, seed=1):
    """The candidate point (of n_try uniform ones) at which the site nearest to an atom, by the minimum
    image, is farthest from it: where the solute with these body offsets clashes least with the water."""
    box = float(a["box"])
    pts = np.random.default_rng(seed).random((n_try, 3)) * box
    worst = np.full(n_try, np.inf)
    for off in np.asarray(offsets, dtype=float):
        for k0 in range(0, n_try, 500):
            d = (pts[k0:k0 + 500] + off)[:, None, :] - np.asarray(a["coords"])[None, :, :]
            d -= box * np.round(d / box)
            worst[k0:k0 + 500] = np.minimum(worst[k0:k0 + 500], np.sqrt((d * d).sum(2)).min(1))
    return pts[int(worst.argmax())]


def sample(a, sol, mol, args, per_sample):
    """One state point: the chains equilibrated around the solute, then per_sample(out) of every block's
    solute_forces(details=True), averaged over the blocks per replica.  Returns (mean [R, ...], flagged)."""
    R, T, n_mol, box = args.replicas, args.temperature, a["com"].shape[0], a["box"]
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, 5.6 / box, structs.factor,
              10.0, 10.0)
    b.set_option("device_moves", 1)
    b.set_solute(sol, mol)
    tot = b.potential_ewald()                                   # (also builds S(k) of the N + 1 system)
    chains = b.new_chains([t["energy"] for t in tot], [t["virial"] for t in tot], dr_max=0.316555789, dphi_max=0.05)
    b.run_chains(chains, args.equil * n_mol, T, seed=4321, adjust=True, n_threads=2)
    acc, n_ok = None, np.zeros(R)
    for blk in range(1, args.blocks + 1):
        b.run_chains(chains, args.sweeps * n_mol, T, seed=11234 + 1000 * blk, adjust=True, n_threads=2)
        out = b.solute_forces(details=True)
        x = per_sample(out)
        ok = out["flags"] == 0
        acc = np.zeros_like(x) if acc is None else acc
        acc[ok] += x[ok]
        n_ok += ok
    b.close()
    flags = (n_ok == 0).astype(np.uint8)                        # a replica flagged in every block is left out
    return acc / np.maximum(n_ok, 1).reshape((-1,) + (1,) * (acc.ndim - 1)), flags


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--sweeps", type=int, default=2, help="sweeps (N_mol trial moves) per block")
    ap.add_argument("--equil", type=int, default=6, help="sweeps before the first sample")
    ap.add_argument("--temperature", type=float, default=298.15)
    args = ap.parse_args()
    a = mio.load_nist_fixture(4, "unwrapped")
    c = cavity(a, np.zeros((1, 3)))

    # ---- charging a cation ----
    q_full = np.array([ION["cation"][0]])
    means, errs = [], []
    print("charging a cation: lambda, <q phi> (K), error")
    for lam in LAMBDAS:
        sol = solute(a, ["cation"], lam * q_full, np.zeros((1, 3)))
        x, flags = sample(a, sol, np.vstack([c, c]), args, lambda out: observables.charging_derivative(out["phi"], q_full))
        m, e, n = observables.solute_mean_force(x, flags)
        means.append(float(m))
        errs.append(float(e))
        print(f"  {lam:5.2f} {m:12.1f} {e:8.1f}   ({n} replicas)")
    dA, dA_err = observables.charging_free_energy(LAMBDAS, means, errs)
    print(f"charging free energy {dA:.1f} +- {dA_err:.1f} K = {dA * 0.0019872:.2f} kcal/mol "
          "(periodic images included, no background)")

    # ---- an ion pair along x ----
    f_mean, f_err = [], []
    print("ion pair: d (A), solvent's mean force along the axis (K/A, > 0 pushes apart), error")
    for d in SEPARATIONS:
        off = np.array([[-0.5 * d, 0.0, 0.0], [0.5 * d, 0.0, 0.0]])
        sol = solute(a, ["cation", "anion"], [ION["cation"][0], ION["anion"][0]], off)
        c = cavity(a, off)
        mol = np.vstack([c + off, c])

        def axial(out, sol=sol, mol=mol):
            return observables.pair_mean_force(out["site_lj"] + sol.charge[None, :, None] * out["field"], mol, 0, 1)
        x, flags = sample(a, sol, mol, args, axial)
        m, e, n = observables.solute_mean_force(x, flags)
        f_mean.append(float(m))
        f_err.append(float(e))
        print(f"  {d:5.2f} {m:12.1f} {e:8.1f}   ({n} replicas)")
    W, W_err = observables.pmf_from_mean_force(SEPARATIONS, f_mean, f_err)
    print("solvent's part of the PMF, W(d) - W(d_max) (K); add the direct cation-anion interaction:")
    for d, w, we in zip(SEPARATIONS, W, W_err):
        print(f"  {d:5.2f} {w:12.1f} {we:8.1f}")


if __name__ == "__main__":
    main()
