#!/usr/bin/env python3
"""Insertion of foreign solutes (mmc_batch_widom_solute) against insertion of the batch's own water
(mmc_batch_widom), on one GPU, one process: 750-molecule SPC/E (NIST config 4) at R = 4096 and at
bench.py's headline replica count, 750 insertions per replica and call.

Per size, after a warm-up of every side, --rounds rounds of one synchronous call each of
  (a) widom: the kernel specialised for the batch's three-site molecule;
  (b) widom_solute with water as the solute (three sites, charged): the same energies by the
      generic S-site kernel;
  (c) widom_solute with a neutral one-site solute (united-atom methane): no reciprocal part;
  (d) widom_solute with an 11-site solute (the monoethanolamine of the reference's mixture deck, its
      LJ rows mixed against SPC/E),
taken in turn (a, b, c, d, a, ...) so that drift hits all alike.  Every call returns after the
device is done and the sums are on the host.  The JSON has every sample, medians and the spread
(min, max), and the ratios of the medians to (a) and of (c) to (b); nothing is enforced.

    python3 scripts/solute_bench.py [--replicas 4096,61440] [--rounds 7] [--out profiles/solute_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import io as mio, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402

T, DR, DPHI, RCUT = 298.15, 0.316555789, 0.05, 10.0
N_INSERT = 750
DECKS = os.path.join(ROOT, "tests", "golden", "decks")


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    return {"ms": ms, "median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def solutes(a, offsets):
    """water, methane and MEA against the three atom slots of the SPC/E batch."""
    st = np.asarray(a["atype"][:3]) - 1
    e_w, s_w = np.diag(a["eps"])[st], np.diag(a["sig"])[st]

    def rows(eps_site, sig_site):   # structs.Tables' mixing
        eps_site, sig_site = np.asarray(eps_site, dtype=float), np.asarray(sig_site, dtype=float)
        return np.sqrt(eps_site[:, None] * e_w[None, :]), (sig_site[:, None] + s_w[None, :]) / 2

    water = structs.Solute("water", offsets, a["charge"][:3], a["eps"][st][:, st], a["sig"][st][:, st])
    methane = structs.Solute("methane", np.zeros((1, 3)), [0.0], *rows([147.9], [3.73]))
    top = mio.ReadTopFile(os.path.join(DECKS, "topol.top"), substitutions={"SOLNUMBER": 1})
    m = mio.system_from_decks(mio.ReadPDB(os.path.join(DECKS, "mea.pdb")), top)
    types = [top["atomtypes"][t - 1] for t in m["atype"]]
    mea = structs.Solute("mea", m["coords"] - m["com"][0], m["charge"],
                         *rows([t["epsilon"] / mio.R_GAS for t in types], [t["sigma"] * 10.0 for t in types]))
    return water, methane, mea


def one_size(a, R, rounds):
    box = float(a["box"])
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, 5.6 / box,
              structs.factor, RCUT, RCUT)
    b.set_option("device_moves", 1)
    e = b.potential_ewald(as_array=True)["energy"].copy()
    e, _ = b.run(64, T, DR, DPHI, seed=11, energies=e, n_groups=2, n_threads=1)   # replicas diverge
    water, methane, mea = solutes(a, b.widom_offsets)
    sides = [("widom", lambda: b.widom(N_INSERT, T, seed=5)),
             ("solute_water", lambda: b.widom_solute(water, N_INSERT, T, seed=5)),
             ("solute_methane", lambda: b.widom_solute(methane, N_INSERT, T, seed=5)),
             ("solute_mea", lambda: b.widom_solute(mea, N_INSERT, T, seed=5))]
    out = {}
    for _ in range(2):                      # warm-up: code load, first allocations
        for name, fn in sides:
            out[name] = fn()
    # the generic kernel on water draws widom's molecules: the same overlaps, the same sums to rounding
    assert np.array_equal(out["widom"][1], out["solute_water"][1])
    assert np.all(np.abs(out["widom"][0] - out["solute_water"][0]) <= 1e-9 * np.abs(out["widom"][0]))
    ms = {name: [] for name, _ in sides}
    for _ in range(rounds):
        for name, fn in sides:
            ms[name].append(timed(fn)[0])
    b.close()
    res = {"replicas": R, "n_mol": int(a["com"].shape[0]), "n_insert": N_INSERT,
           "sites": {"solute_water": 3, "solute_methane": 1, "solute_mea": int(mea.n_sites)}}
    for name, _ in sides:
        res[name] = summary(ms[name])
        res[name]["insertions_per_s"] = N_INSERT * R / (res[name]["median_ms"] * 1e-3)
        res[name]["overlap_share"] = float(out[name][1].sum() / (N_INSERT * R))
    med = {name: res[name]["median_ms"] for name, _ in sides}
    res["b_over_a_median"] = med["solute_water"] / med["widom"]
    res["c_over_b_median"] = med["solute_methane"] / med["solute_water"]
    res["d_over_a_median"] = med["solute_mea"] / med["widom"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", default="4096,61440")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    a = mio.load_nist_fixture(4, "unwrapped")
    res = {"bench": "solute", "system": "SPC/E, NIST configuration 4",
           "sizes": [one_size(a, int(r), args.rounds) for r in args.replicas.split(",")]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
