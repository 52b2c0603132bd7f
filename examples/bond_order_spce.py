#!/usr/bin/env python3
"""Is there ice in the box?  Liquid SPC/E chains (NIST configuration 4, as examples/nvt_spce.py runs
them) and chains started from a proton-ordered cubic-ice (diamond) lattice, side by side: after a few
sweeps, once per sweep, Steinhardt's neighbour-averaged qbar_6 over 16 neighbours, the CHILL+ bond
correlations c_3 over the four nearest neighbours, the CHILL+ classes and the largest cluster of
solid-like molecules of every replica (mmc_batch_bond_order).  The chains are not disturbed.

    python3 examples/bond_order_spce.py [--replicas 64] [--equil 5] [--sweeps 10] [--cells 4]

Prints, for each of the two batches, the mean and the spread of qbar_6, the shares of staggered and
eclipsed bonds, the populations of the six classes and the largest nucleus (mean and maximum over
chains and sweeps).  No assertion on the values.  Needs an MI355X.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import io as mio, observables, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402

TETRA = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) / np.sqrt(3.0)
MASS = np.array([15.9994, 1.008, 1.008])


def cubic_ice(cells, r_oo=2.75, r_oh=1.0):
    """(com [N, 3], coords [3 N, 3], box) of 8 cells^3 waters on a diamond lattice with O-O = r_oo.
    The molecules of one fcc sublattice have their bonds along +TETRA and donate along the first two,
    those of the other along -TETRA and donate along the last two: one hydrogen on every bond."""
    cell = 4.0 * r_oo / np.sqrt(3.0)
    fcc = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    mols = []
    for i in range(cells):
        for j in range(cells):
            for k in range(cells):
                for f in fcc:
                    o = (np.array([i, j, k]) + f) * cell
                    mols.append([o, o + r_oh * TETRA[0], o + r_oh * TETRA[1]])
                    o = o + 0.25 * cell
                    mols.append([o, o - r_oh * TETRA[2], o - r_oh * TETRA[3]])
    coords = np.array(mols)                                             # [N, 3, 3]
    com = (coords * MASS[None, :, None]).sum(1) / MASS.sum()
    return com, coords.reshape(-1, 3), cells * cell


def sample(b, n_mol, T, equil, sweeps, seed):
    tot = b.potential_ewald()
    chains = b.new_chains([t["energy"] for t in tot], [t["virial"] for t in tot], dr_max=0.316555789, dphi_max=0.05)
    if equil:
        b.run_chains(chains, equil * n_mol, T, seed=seed, adjust=True, n_threads=2)
    acc, classes, largest = None, [], []
    for s in range(sweeps):
        b.run_chains(chains, n_mol, T, seed=seed + 1 + s, adjust=False, n_threads=2)
        q6 = b.bond_order(l=6, n_nb=16, r_nb=3.5, a=(0.5, 1.0), min_a=7, min_ab=0)
        chill = b.bond_order(details=True)                             # the CHILL+ defaults
        classes.append(observables.chill_plus_classes(chill))
        largest.append(observables.largest_nucleus(chill["stats"]))
        out = dict(qbar6_hist=q6["qbar_hist"], c3_hist=chill["c_hist"], stats=chill["stats"])
        if acc is None:
            acc = out
        else:
            for k in acc:
                acc[k] += out[k]
    return acc, np.array(classes), np.array(largest)


def report(name, n_mol, acc, classes, largest):
    q, p, undefined = observables.steinhardt_distribution(acc["qbar6_hist"])
    w = p / p.sum()
    mean = (w * q).sum()
    print(f"{name}: {n_mol} molecules")
    print(f"  qbar_6: mean {mean:.4f}, standard deviation {np.sqrt((w * (q - mean) ** 2).sum()):.4f} "
          f"(undefined for {undefined:.2e} of the molecules)")
    c, pc, und_c = observables.bond_correlation_distribution(acc["c3_hist"])
    wc = pc / pc.sum()
    print(f"  c_3: staggered (c <= -0.8) {wc[c <= -0.8].sum():.3f}, eclipsed (-0.35 <= c <= 0.25) "
          f"{wc[(c >= -0.35) & (c <= 0.25)].sum():.3f} of the defined bonds ({und_c:.2e} undefined)")
    share = classes.sum((0, 1)) / classes.sum()
    print("  classes: " + ", ".join(f"{k} {v:.3f}" for k, v in zip(observables.CHILL_CLASSES, share)))
    print(f"  solid-like (cubic or hexagonal): {observables.solid_fraction(acc['stats'].sum(0)):.3f} of the molecules; "
          f"largest nucleus: mean {largest.mean():.1f}, maximum {int(largest.max())}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=64)
    ap.add_argument("--equil", type=int, default=5, help="sweeps before sampling")
    ap.add_argument("--sweeps", type=int, default=10, help="sampled sweeps")
    ap.add_argument("--cells", type=int, default=4, help="diamond cells per edge (8 molecules each)")
    ap.add_argument("--temperature", type=float, default=298.15)
    args = ap.parse_args()
    T, R, r_cut = args.temperature, args.replicas, 10.0

    a = mio.load_nist_fixture(4, "unwrapped")
    n_liq, box = a["com"].shape[0], a["box"]
    with Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, 5.6 / box, structs.factor,
               r_cut, r_cut) as b:
        b.set_option("device_moves", 1)
        liquid = sample(b, n_liq, T, args.equil, args.sweeps, 11234)

    com, coords, ice_box = cubic_ice(args.cells)
    n_ice = com.shape[0]
    if n_ice > n_liq or 2.0 * r_cut > ice_box:
        raise SystemExit(f"--cells {args.cells}: {n_ice} molecules in a box of {ice_box:.2f} A; "
                         f"this example needs L >= 20 A and at most {n_liq} molecules (4 cells)")
    with Batch(R, com, coords, a["atype"][:3 * n_ice], a["charge"][:3 * n_ice], a["eps"], a["sig"], ice_box, 5.6 / ice_box,
               structs.factor, r_cut, r_cut) as b:
        b.set_option("device_moves", 1)
        ice = sample(b, n_ice, T, args.equil, args.sweeps, 21234)

    print(f"{R} chains each, {args.equil} + {args.sweeps} sweeps, T = {T} K")
    report(f"liquid (L = {box} A)", n_liq, *liquid)
    report(f"cubic-ice start (L = {ice_box:.3f} A)", n_ice, *ice)


if __name__ == "__main__":
    main()
