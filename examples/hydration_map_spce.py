#!/usr/bin/env python3
"""Hydration maps of a solute held fixed in SPC/E water: where the oxygens and the hydrogens sit around
it, which way the waters point there, and how much each place adds to the water-solute energy
(mmc_batch_hydration_map) -- for a sodium-like cation and for the decks' 11-atom monoethanolamine
(tests/golden/decks: mea.pdb + topol.top), each in its own batch of 750 waters (NIST configuration 4).

    python3 examples/hydration_map_spce.py [--replicas 64] [--blocks 20] [--sweeps 10] [--equil 200]
                                           [--n-half 12] [--cell 0.5] [--solutes cation,mea]

The solute is fixed and the same in every replica, so the laboratory frame is its frame: one cube of
(2 n_half)^3 cells centred on its reference point takes the waters of all R chains, and nothing is
aligned.  The solute is set where it fits best among the cavities of the starting configuration; after
`--equil` sweeps every block of `--sweeps` sweeps ends with one map summed over the replicas, and the
maps are added up over the blocks.  Prints the cells of the largest g_O and g_H with their places, the
shell profile of g_O, the mean <e_z . r^> of the waters of the first shell (e_z the unit bisector, from
the O towards the hydrogens; r^ from the reference point to the cell: +1 = hydrogens outwards, as
around a cation), and the share of <u_sw> that the cube holds.  The numbers are unmeasured until
someone runs this: no assertion on any value.  Needs an MI355X.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import io as mio, observables, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402

DECKS = os.path.join(ROOT, "tests", "golden", "decks")


def make_solutes(a):
    """A cation (q = +1, 65.4 K, 2.35 A) and the deck's MEA against the batch's three atom slots, mixed
    by the reference's rules (structs.Tables)."""
    st = np.asarray(a["atype"][:3]) - 1
    e_w, s_w = np.diag(a["eps"])[st], np.diag(a["sig"])[st]

    def rows(eps_site, sig_site):
        eps_site, sig_site = np.asarray(eps_site, dtype=float), np.asarray(sig_site, dtype=float)
        return np.sqrt(eps_site[:, None] * e_w[None, :]), (sig_site[:, None] + s_w[None, :]) / 2

    cation = structs.Solute("cation", np.zeros((1, 3)), [1.0], *rows([65.4], [2.35]))
    top = mio.ReadTopFile(os.path.join(DECKS, "topol.top"), substitutions={"SOLNUMBER": 1})
    m = mio.system_from_decks(mio.ReadPDB(os.path.join(DECKS, "mea.pdb")), top)
    types = [top["atomtypes"][t - 1] for t in m["atype"]]
    mea = structs.Solute("mea", m["coords"] - m["com"][0], m["charge"],
                         *rows([t["epsilon"] / mio.R_GAS for t in types], [t["sigma"] * 10.0 for t in types]))
    return {"cation": cation, "mea": mea}


def rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def best_fit(a, sol, n_points=40, n_rot=24, seed=1):
    """mol [S + 1][3]: the solute at the place and in the orientation (of the n_points emptiest of 4000
    random points x n_rot random rotations) that keeps its sites farthest from every atom."""
    box, rng = float(a["box"]), np.random.default_rng(seed)
    at = np.asarray(a["coords"])

    def clearance(p):
        d = p[:, None, :] - at[None, :, :]
        d -= box * np.round(d / box)
        return np.sqrt((d * d).sum(2)).min(1)
    pts = rng.random((4000, 3)) * box
    pts = pts[np.argsort(-clearance(pts))[:n_points]]
    best, best_d = None, -1.0
    for c in pts:
        for k in range(n_rot if sol.n_sites > 1 else 1):
            sites = c + sol.offsets @ rotation(rng).T
            d = float(clearance(sites).min())
            if d > best_d:
                best, best_d = np.vstack([sites, c]), d
    return best, best_d


def report(sol, maps, frames, n_mol, box, n_half, cell):
    ch = {name: maps[k] for k, name in enumerate(Batch.HYDRATION_CHANNELS)}
    cells = (2 * n_half) ** 3
    centres = observables.hydration_map_centres(n_half, cell)
    g_o = observables.hydration_density(ch["O"], frames, n_mol, box ** 3, cell)
    g_h = observables.hydration_density(ch["H1"] + ch["H2"], 2 * frames, n_mol, box ** 3, cell)
    for name, g in (("g_O", g_o), ("g_H", g_h)):
        k = np.unravel_index(int(np.argmax(g)), g.shape)
        x = centres[k]
        print(f"  largest {name} = {g[k]:7.2f} in the cell at ({x[0]:+.2f}, {x[1]:+.2f}, {x[2]:+.2f}) A, "
              f"{np.linalg.norm(x):.2f} A from the reference point")
    dr = cell
    r, prof, n_c = observables.hydration_radial_average(g_o, n_half, cell, dr)
    k_peak = int(np.nanargmax(prof))
    k_min = k_peak + int(np.nanargmin(prof[k_peak:min(k_peak + int(2.5 / dr) + 1, prof.shape[0])]))
    print("  shell average of g_O: " + ", ".join(f"{r[k]:.2f} A {prof[k]:.2f}" for k in range(prof.shape[0]) if n_c[k]))
    r_shell = (k_min + 1) * dr
    rr = np.sqrt((centres * centres).sum(-1))
    shell = rr < r_shell
    p_sum = np.moveaxis(np.asarray(maps[3:6, :cells], dtype=float).reshape(3, *rr.shape), 0, -1) / observables.HMAP_VEC_SCALE
    n_o = np.asarray(ch["O"][:cells], dtype=float).reshape(rr.shape)
    radial = (p_sum * centres).sum(-1) / rr
    print(f"  first shell (cell centres within {r_shell:.2f} A, the first minimum of the shell average): "
          f"{n_o[shell].sum() / frames:.2f} waters, <e_z . r^> = {radial[shell].sum() / max(n_o[shell].sum(), 1.0):+.3f}")
    pol = observables.hydration_polarisation(maps[3:6], ch["O"])
    k = np.unravel_index(int(np.argmax(g_o)), g_o.shape)
    print(f"  <e_z> in the cell of the largest g_O: ({pol[k][0]:+.2f}, {pol[k][1]:+.2f}, {pol[k][2]:+.2f})")
    per_water, per_vol = observables.hydration_energy(maps[6:8], ch["O"], cell, frames)
    inside = per_vol.sum() * cell ** 3
    outside = float(ch["u_lj"][cells] + ch["u_real"][cells]) / observables.HMAP_E_SCALE / frames
    k = np.unravel_index(int(np.nanargmin(np.where(n_o > 0.001 * frames, per_water, np.nan))), per_water.shape)
    x = centres[k]
    print(f"  <u_sw> = {inside + outside:.1f} K, of which the cube of {2 * n_half * cell:.1f} A holds {inside:.1f} K "
          f"({100.0 * inside / (inside + outside):.1f} %); {int(ch['u_lj'][cells + 1])} waters left out of the energy maps, "
          f"{int(ch['px'][cells + 1])} without a bisector")
    print(f"  lowest mean u_sw of a water: {per_water[k]:.0f} K = {per_water[k] * structs.R:.1f} kJ/mol in the cell at "
          f"({x[0]:+.2f}, {x[1]:+.2f}, {x[2]:+.2f}) A (cells with more than one water in 1000 frames)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--sweeps", type=int, default=10, help="sweeps (N_mol trial moves) per block")
    ap.add_argument("--equil", type=int, default=200, help="sweeps before the first map")
    ap.add_argument("--n-half", type=int, default=12)
    ap.add_argument("--cell", type=float, default=0.5)
    ap.add_argument("--solutes", default="cation,mea")
    ap.add_argument("--temperature", type=float, default=298.15)
    args = ap.parse_args()
    T, R = args.temperature, args.replicas

    a = mio.load_nist_fixture(4, "unwrapped")
    n_mol, box, r_cut = a["com"].shape[0], a["box"], 10.0
    solutes = make_solutes(a)
    for name in args.solutes.split(","):
        sol = solutes[name]
        mol, clear = best_fit(a, sol)
        b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, 5.6 / box,
                  structs.factor, r_cut, r_cut)
        b.set_option("device_moves", 1)
        b.set_solute(sol, mol)
        tot = b.potential_ewald()                               # (also builds S(k) of the N + 1 system)
        chains = b.new_chains([t["energy"] for t in tot], [t["virial"] for t in tot], dr_max=0.316555789, dphi_max=0.05)
        b.run_chains(chains, args.equil * n_mol, T, seed=4321, adjust=True, n_threads=2)
        maps = np.zeros((8, (2 * args.n_half) ** 3 + 2), dtype=np.int64)
        for blk in range(1, args.blocks + 1):
            b.run_chains(chains, args.sweeps * n_mol, T, seed=11234 + 1000 * blk, adjust=True, n_threads=2)
            maps += b.hydration_map(args.n_half, args.cell)
        b.close()
        print(f"{sol.name} ({sol.n_sites} sites, net charge {sol.charge.sum():+.2f}) in {n_mol} SPC/E, {R} replicas x "
              f"{args.blocks} maps of {2 * args.n_half}^3 cells of {args.cell} A; set {clear:.2f} A clear of every atom")
        report(sol, maps, R * args.blocks, n_mol, box, args.n_half, args.cell)


if __name__ == "__main__":
    main()
