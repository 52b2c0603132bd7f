#!/usr/bin/env python3
"""One shell_order call (sorted neighbour lists, rank histograms, LSI, zeta and O-O-O angles of every
molecule, mmc_batch_shell_order) against one local_order(400) call and one rdf_sites(200) call, on one
GPU, one process: 750-molecule SPC/E (NIST config 4) at R = 4096 and at bench.py's headline replica
count.

Per size, after a warm-up of every side, --rounds rounds of
  full       shell_order with its defaults (r_list 6, r_lsi 3.7, r_ang 3.3, r_hb 3.5, 30 deg; 8 rank rows
             of 300 bins, 200 LSI, 180 angle and 200 zeta bins), summed histograms and the sums;
  hists      the same without the sums (no per-molecule arrays, no k_local_qsum);
  scan       the scan alone: r_list = 0.5 A, so every list is empty, and one counter;
  list       scan, lists, sort and the rank histograms: the defaults with only rank_hist asked for;
  hists_small, list_small
             hists and list with a tenth of the bins (30, 20, 18, 20): the same work per molecule with
             counters small enough for four waves per workgroup and every workgroup resident -- what
             the LDS the default bins take costs;
  lsi_3.7    r_list = 3.7 A, r_lsi = 3.5 A, only lsi_hist (with r_lsi = r_list no LSI would be defined:
             the neighbour beyond r_lsi has to be listed);
  local      one local_order(400) call, summed output: the yardstick, the same O(N^2) scan and staging;
  rdf        one rdf_sites(200) call,
taken in turn (full, hists, ..., rdf, full, ...) so that drift hits all alike.  Every call is
synchronous: it returns after the device is done and the output is on the host.  The JSON has every
sample, medians and the spread (min, max), the ratios to local_order, the share of the scan, and the
frame's <d5>, <I>, <zeta> and flagged count.

    python3 scripts/shell_order_bench.py [--replicas 4096,61440] [--rounds 7] [--out profiles/shell_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import _lib, io as mio, observables as obs, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402

T, DR, DPHI, RCUT = 298.15, 0.316555789, 0.05, 10.0
Q_BINS, NUMBINS = 400, 200
DEFAULTS = dict(r_list=6.0, r_lsi=3.7, r_ang=3.3, r_hb=3.5, theta_deg=30.0, n_rank=8, r_bins=300, lsi_bins=200,
                lsi_max=0.4, ang_bins=180, zeta_bins=200, zeta_lo=-1.5, zeta_hi=2.5)
HISTS = ("rank_hist", "lsi_hist", "ang_hist", "zeta_hist")
SMALL = dict(r_bins=30, lsi_bins=20, ang_bins=18, zeta_bins=20)   # a tenth of the counters: four waves per workgroup


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    return {"ms": ms, "median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def partial_call(b, want, **kw):
    """The C call with only the outputs named in `want` (of HISTS and "sums"), summed histograms."""
    p = dict(DEFAULTS, **kw)
    shape = dict(rank_hist=(p["n_rank"], p["r_bins"] + 1), lsi_hist=(p["lsi_bins"] + 1,), ang_hist=(p["ang_bins"] + 1,),
                 zeta_hist=(p["zeta_bins"] + 1,))
    res = {k: np.zeros(shape[k], dtype=np.uint64) for k in HISTS if k in want}
    if "sums" in want:
        res["sums"] = np.zeros((b.R, 4))
    u64, dbl = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    _lib.check(_lib.lib().mmc_batch_shell_order(
        b._h, p["r_list"], p["r_lsi"], p["r_ang"], p["r_hb"], float(np.cos(np.deg2rad(p["theta_deg"]))), p["n_rank"],
        p["r_bins"], p["lsi_bins"], p["lsi_max"], p["ang_bins"], p["zeta_bins"], p["zeta_lo"], p["zeta_hi"], 0,
        *[res[k].ctypes.data_as(u64) if k in res else None for k in HISTS], None,
        res["sums"].ctypes.data_as(dbl) if "sums" in res else None, None, None, None, None))
    return res


def one_size(a, R, rounds):
    box = float(a["box"])
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, 5.6 / box,
              structs.factor, RCUT, RCUT)
    b.set_option("device_moves", 1)
    e = b.potential_ewald(as_array=True)["energy"].copy()
    e, _ = b.run(64, T, DR, DPHI, seed=11, energies=e, n_groups=2, n_threads=1)   # replicas diverge

    sides = {
        "full": lambda: b.shell_order(),
        "hists": lambda: partial_call(b, HISTS),
        "scan": lambda: partial_call(b, ("rank_hist",), r_list=0.5, r_lsi=0.5, r_ang=0.5, r_hb=0.5, n_rank=1, r_bins=1),
        "list": lambda: partial_call(b, ("rank_hist",)),
        "hists_small": lambda: partial_call(b, HISTS, **SMALL),
        "list_small": lambda: partial_call(b, ("rank_hist",), **SMALL),
        "lsi_3.7": lambda: partial_call(b, ("lsi_hist",), r_list=3.7, r_lsi=3.5),
        "local": lambda: b.local_order(Q_BINS),
        "rdf": lambda: b.rdf_sites(NUMBINS),
    }
    out = {}
    for _ in range(2):                      # warm-up: code load, first allocations
        for k, fn in sides.items():
            out[k] = fn()
    n = a["com"].shape[0]
    so = out["full"]
    assert np.all(so["rank_hist"].sum(1) + so["flagged"].sum() == R * n)
    assert all(np.array_equal(out["hists"][k], so[k]) for k in HISTS)
    assert np.array_equal(out["list"]["rank_hist"], so["rank_hist"]) and out["scan"]["rank_hist"][0, 1] == R * n
    ms = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            ms[k].append(timed(fn)[0])
    b.close()
    res = {"replicas": R, "n_mol": int(n), "defaults": DEFAULTS, "q_bins": Q_BINS, "numbins": NUMBINS}
    res.update({k: summary(v) for k, v in ms.items()})
    med = {k: res[k]["median_ms"] for k in sides}
    r, pk, beyond = obs.neighbour_distance_distributions(so["rank_hist"], DEFAULTS["r_list"])
    theta, p_theta, mean_cos = obs.ooo_angle_distribution(so["ang_hist"])
    res.update(full_over_local=med["full"] / med["local"], hists_over_local=med["hists"] / med["local"],
               lsi_3_7_over_local=med["lsi_3.7"] / med["local"], full_over_rdf=med["full"] / med["rdf"],
               scan_share_of_full=med["scan"] / med["full"], list_share_of_full=med["list"] / med["full"],
               scan_over_local=med["scan"] / med["local"],
               hists_small_over_local=med["hists_small"] / med["local"],
               oo_distances_per_s_scan=n * (n - 1) * R / (med["scan"] * 1e-3),
               flagged=int(so["flagged"].sum()), d5_mean=float((pk[4] * r).sum() * (r[1] - r[0])),
               d5_beyond=float(beyond[4]), lsi_mean=float(obs.lsi_mean(so["sums"].sum(0))),
               zeta_mean=float(obs.zeta_mean(so["sums"].sum(0))), angle_peak_deg=float(theta[int(np.argmax(p_theta))]),
               mean_cos=float(mean_cos))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", default="4096,61440")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    a = mio.load_nist_fixture(4, "unwrapped")
    res = {"bench": "shell_order", "system": "SPC/E, NIST configuration 4",
           "sizes": [one_size(a, int(r), args.rounds) for r in args.replicas.split(",")]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
