#!/usr/bin/env python3
"""The pressure of SPC/E water from R NVT chains as examples/nvt_spce.py runs them (Loop(),
Ewald/main.jl:460-696), by virtual volume moves: after equilibration, once per sweep, every replica's
energy change under the NPT move's own rescale to V + dv and V - dv (mmc_batch_volume_perturb,
read-only), accumulated as w = (V'/V)^N exp(-dU / T).  beta P = ln <w> / dv is the pressure an NPT
chain of this code would equilibrate this state to (truncated LJ, no tail correction).  The chains
are not disturbed.

    python3 examples/pressure_spce.py [--replicas 64] [--equil 20] [--sweeps 40] [--dv 50]

Prints the two-sided perturbation pressure with the standard error over chains, the pooled value,
the one-sided values, and beside them the status line's figure (main.jl:677: a hard-coded ideal
term plus virial / V, kept for parity; its Coulomb virial ignores the rigid molecules' constraint
forces).  No assertion on the values.  Needs an MI355X.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import io as mio, observables, structs  # noqa: E402
from metropolismontecarlo_amd.device import REFERENCE_IDEAL_TERM, Batch  # noqa: E402

K_PER_A3_IN_BAR = 138.0649  # k_B / A^3 in bar


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=64)
    ap.add_argument("--equil", type=int, default=20, help="sweeps before sampling")
    ap.add_argument("--sweeps", type=int, default=40, help="sampled sweeps")
    ap.add_argument("--dv", type=float, default=50.0, help="test volume change in A^3")
    ap.add_argument("--temperature", type=float, default=298.15)
    args = ap.parse_args()
    T, R = args.temperature, args.replicas

    a = mio.load_nist_fixture(4, "unwrapped")
    n_mol, box, r_cut = a["com"].shape[0], a["box"], 10.0
    V = box ** 3
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box,
              5.6 / box, structs.factor, r_cut, r_cut)
    b.set_option("device_moves", 1)
    tot = b.potential_ewald()
    chains = b.new_chains([t["energy"] for t in tot], [t["virial"] for t in tot],
                          dr_max=0.316555789, dphi_max=0.05)
    b.run_chains(chains, args.equil * n_mol, T, seed=11234, adjust=True, n_threads=2)
    dvs = [args.dv, -args.dv]
    boltz = np.zeros((R, 2))
    n_ovl = np.zeros((R, 2), dtype=np.int64)
    line = np.zeros(R)
    for s in range(args.sweeps):
        b.run_chains(chains, n_mol, T, seed=20000 + s, adjust=False, n_threads=2)
        b.volume_perturb(T, dv=dvs, boltz_sum=boltz, n_overlap=n_ovl)
        line += REFERENCE_IDEAL_TERM + chains["virial"] / V
    b.close()

    p = observables.pressure_from_volume_perturbation(boltz, args.sweeps, dvs, T)

    def with_error(x):                                   # mean over chains and its standard error
        return x.mean(), (x.std(ddof=1) / np.sqrt(R) if R > 1 else float("nan"))

    print(f"{R} chains, {args.sweeps} sampled sweeps of {n_mol} molecules, T = {T} K, L = {box} A, "
          f"dv = +-{args.dv} A^3 ({100 * args.dv / V:.2f} % of V); weights forced to 0: {int(n_ovl.sum())}")
    m, e = with_error(p["two_sided_per_replica"][:, 0])
    print(f"perturbation pressure, two-sided: {m:.5f} +- {e:.5f} K/A^3 = {m * K_PER_A3_IN_BAR:.0f} +- "
          f"{e * K_PER_A3_IN_BAR:.0f} bar (mean of the chains' own estimates)")
    print(f"  pooled over chains: {p['two_sided_pooled'][0]:.5f} K/A^3 = "
          f"{p['two_sided_pooled'][0] * K_PER_A3_IN_BAR:.0f} bar")
    for k, dv in enumerate(dvs):
        m, e = with_error(p["per_replica"][:, k])
        print(f"  one-sided dv = {dv:+.1f}: {m:.5f} +- {e:.5f} K/A^3")
    m, e = with_error(line / args.sweeps)
    print(f"status-line figure (ideal term {REFERENCE_IDEAL_TERM} + virial / V): {m:.5f} +- {e:.5f}")


if __name__ == "__main__":
    main()
