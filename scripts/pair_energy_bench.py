#!/usr/bin/env python3
"""One pair_energy call (pair-energy distributions, mmc_batch_pair_energy) against one rdf_sites call
(the six site-site histograms, mmc_batch_rdf_sites) and one orient_corr call (mmc_batch_orient_corr),
on one GPU, one process: 750-molecule SPC/E (NIST config 4) at R = 4096 and at bench.py's headline
replica count, the shapes of scripts/orient_bench.py.

Per size, after a warm-up of all three, --rounds rounds of
  (a) one pair_energy(200, r_max = L / 2, 120 energy bins over [-4000, 2000) K, u_hb = -1132.2 K)
      call, summed output: N (N - 1) / 2 site-0 distances per replica; the pairs within L / 2 (about
      half) also take nine atom-pair distances with a refined reciprocal square root each, the
      Lennard-Jones terms, three more 64-bit LDS atomics and the per-molecule bond counts;
  (b) one rdf_sites(200, r_max = L / 2) call: 9 N (N - 1) / 2 site-site distances per replica, six
      32-bit rows;
  (c) one orient_corr(200, r_max = L / 2) call: the same pair loop as (a) with three dot products and
      a reciprocal in place of the energies,
taken alternately (a, b, c, a, b, c, ...) so that drift hits all alike.  Every call is synchronous: it
returns after the device is done and the output is on the host.  The JSON has every sample, medians
and the spread (min, max), the ratios of the medians, the fraction of pairs within L / 2 and the
frame's energetic bonds per molecule and pair energy per molecule.  The yardsticks are (b) and (c) of
the same run; no ratio is a bar.

    python3 scripts/pair_energy_bench.py [--replicas 4096,61440] [--rounds 7] [--out profiles/pair_energy_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import io as mio, observables as obs, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402

T, DR, DPHI, RCUT = 298.15, 0.316555789, 0.05, 10.0
NUMBINS, E_BINS, U_LO, U_HI, U_HB = 200, 120, -4000.0, 2000.0, -1132.2


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    return {"ms": ms, "median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def one_size(a, R, rounds):
    box = float(a["box"])
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, 5.6 / box,
              structs.factor, RCUT, RCUT)
    b.set_option("device_moves", 1)
    e = b.potential_ewald(as_array=True)["energy"].copy()
    e, _ = b.run(64, T, DR, DPHI, seed=11, energies=e, n_groups=2, n_threads=1)   # replicas diverge

    def side_a():
        return b.pair_energy(NUMBINS, box / 2, E_BINS, U_LO, U_HI, U_HB)

    def side_b():
        return b.rdf_sites(NUMBINS, box / 2)

    def side_c():
        return b.orient_corr(NUMBINS, box / 2)

    for _ in range(2):                      # warm-up: code load, first allocations
        pe, six, oc = side_a(), side_b(), side_c()
    n = a["com"].shape[0]
    pairs = n * (n - 1) // 2 * R
    assert pe.rows[0].sum() == pairs and np.array_equal(pe.rows[0], oc[0])
    assert np.array_equal(pe.rows[0, :-1], six[0].astype(np.int64)) and int(pe.nhb.sum()) == n * R
    ta, tb, tc = [], [], []
    for _ in range(rounds):
        ta.append(timed(side_a)[0])
        tb.append(timed(side_b)[0])
        tc.append(timed(side_c)[0])
    b.close()
    in_range = int(pe.rows[0, :-1].sum())
    res = {"replicas": R, "n_mol": int(n), "numbins": NUMBINS, "r_max": box / 2, "n_ebins": E_BINS, "u_hb": U_HB,
           "pair_energy": summary(ta), "rdf_sites_six_rows": summary(tb), "orient_corr": summary(tc),
           "pairs_in_range_fraction": float(in_range / pairs), "flagged": int(pe.flagged[0]),
           "energetic_bonds_per_molecule": float(obs.energetic_hbonds(pe.nhb)[1]),
           "pair_energy_per_molecule_within_r_max_K": float(obs.pair_energy_profile(pe.rows, n, R)[2][-1])}
    res["a_over_b_median"] = res["pair_energy"]["median_ms"] / res["rdf_sites_six_rows"]["median_ms"]
    res["a_over_c_median"] = res["pair_energy"]["median_ms"] / res["orient_corr"]["median_ms"]
    res["pairs_per_s_a"] = pairs / (res["pair_energy"]["median_ms"] * 1e-3)
    res["atom_pairs_in_range_per_s_a"] = 9 * in_range / (res["pair_energy"]["median_ms"] * 1e-3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", default="4096,61440")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    a = mio.load_nist_fixture(4, "unwrapped")
    res = {"bench": "pair_energy", "system": "SPC/E, NIST configuration 4",
           "sizes": [one_size(a, int(r), args.rounds) for r in args.replicas.split(",")]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
