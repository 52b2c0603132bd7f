#!/usr/bin/env python3
"""One voronoi call (the Voronoi cell of every oxygen: volumes, asphericity, geometric neighbours,
mmc_batch_voronoi) against one shell_order() call, on one GPU, one process: 750-molecule SPC/E (NIST
config 4) at R = 4096 and at bench.py's headline replica count, after 64 moves.

Per size, after a warm-up of every side, --rounds rounds of
  full_7.0   voronoi with its defaults (r_list 7 A; 200 volume, 200 asphericity and 280 distance bins),
             summed histograms and the sums;
  full_7.5   the same with r_list = 7.5 A: longer lists, fewer open cells;
  hists      the defaults without the sums (no per-molecule arrays, no k_voronoi_sums);
  lists      the scan and sort alone: shell_order's scan, lists, sort and one rank row at r_list = 7 A,
             the part the two kernels share statement for statement (voronoi itself has no output that
             does not need the clipping: the flags do);
  flags      every output NULL but flagged: the clipping without any reduction or histogram;
  no_prune   full_7.0 with option "voronoi_prune" = 0: every face walks every listed plane (same bits);
  details    (R <= --details-max only) the defaults with the per-molecule outputs, 1 KiB a molecule
             across the bus;
  shell      one shell_order() call with its defaults: the yardstick,
taken in turn so that drift hits all alike.  Every call is synchronous: it returns after the device is
done and the output is on the host.  The JSON has every sample, medians and the spread (min, max), the
ratios to shell_order, what the pruning rule saves, and the frame's flag fractions, <V>, <eta>, <faces>.

    python3 scripts/voronoi_bench.py [--replicas 4096,61440] [--rounds 7] [--out profiles/voronoi_bench.json]
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
DEFAULTS = dict(r_list=7.0, area_min=0.0, v_bins=200, v_max=80.0, eta_bins=200, eta_max=3.0, r_bins=280)
HISTS = ("vol_hist", "eta_hist", "face_hist", "side_hist", "nbr_hist")


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    return {"ms": ms, "median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def partial_call(b, want, **kw):
    """The C call with only the outputs named in `want` (of HISTS, "flagged" and "sums"), summed histograms."""
    p = dict(DEFAULTS, **kw)
    shape = dict(vol_hist=(p["v_bins"] + 1,), eta_hist=(p["eta_bins"] + 1,), face_hist=(65,), side_hist=(17,),
                 nbr_hist=(p["r_bins"] + 1,), flagged=(b.R, 3))
    res = {k: np.zeros(shape[k], dtype=np.uint64) for k in HISTS + ("flagged",) if k in want}
    if "sums" in want:
        res["sums"] = np.zeros((b.R, 8))
    u64, dbl = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    _lib.check(_lib.lib().mmc_batch_voronoi(
        b._h, p["r_list"], p["area_min"], p["v_bins"], p["v_max"], p["eta_bins"], p["eta_max"], p["r_bins"], 0,
        *[res[k].ctypes.data_as(u64) if k in res else None for k in HISTS + ("flagged",)],
        res["sums"].ctypes.data_as(dbl) if "sums" in res else None, None, None, None, None, None))
    return res


def shell_lists(b, r_list):
    """shell_order's scan, lists, sort and one rank row at r_list: what the two calls share."""
    rank = np.zeros((1, 2), dtype=np.uint64)
    u64 = C.POINTER(C.c_uint64)
    _lib.check(_lib.lib().mmc_batch_shell_order(
        b._h, r_list, r_list, r_list, r_list, 1.0, 1, 1, 1, 1.0, 1, 1, 0.0, 1.0, 0, rank.ctypes.data_as(u64),
        None, None, None, None, None, None, None, None, None))
    return rank


def no_prune(b):
    b.set_option("voronoi_prune", 0)
    try:
        return b.voronoi()
    finally:
        b.set_option("voronoi_prune", 1)


def one_size(a, R, rounds, details_max):
    box = float(a["box"])
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, 5.6 / box,
              structs.factor, RCUT, RCUT)
    b.set_option("device_moves", 1)
    e = b.potential_ewald(as_array=True)["energy"].copy()
    e, _ = b.run(64, T, DR, DPHI, seed=11, energies=e, n_groups=2, n_threads=1)   # replicas diverge

    sides = {
        "full_7.0": lambda: b.voronoi(),
        "full_7.5": lambda: b.voronoi(r_list=7.5),
        "hists": lambda: partial_call(b, HISTS + ("flagged",)),
        "lists": lambda: shell_lists(b, DEFAULTS["r_list"]),
        "flags": lambda: partial_call(b, ("flagged",)),
        "no_prune": lambda: no_prune(b),
        "shell": lambda: b.shell_order(),
    }
    if R <= details_max:
        sides["details"] = lambda: b.voronoi(details=True)
    out = {}
    for _ in range(2):                      # warm-up: code load, first allocations
        for k, fn in sides.items():
            out[k] = fn()
    n = a["com"].shape[0]
    vo = out["full_7.0"]
    assert vo["vol_hist"].sum() + vo["flagged"].sum() >= R * n and vo["vol_hist"].sum() == vo["sums"][:, 0].sum()
    assert all(np.array_equal(out["hists"][k], vo[k]) for k in HISTS + ("flagged",))
    assert np.array_equal(out["flags"]["flagged"], vo["flagged"])
    assert all(np.array_equal(out["no_prune"][k].view(np.uint8), vo[k].view(np.uint8)) for k in vo)
    ms = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            ms[k].append(timed(fn)[0])
    b.close()
    res = {"replicas": R, "n_mol": int(n), "defaults": DEFAULTS}
    res.update({k: summary(v) for k, v in ms.items()})
    med = {k: res[k]["median_ms"] for k in sides}

    def frame(o):
        v, eta, faces = obs.voronoi_means(o["sums"].sum(0))
        fl = o["flagged"].sum(0) / float(R * n)
        return dict(cap_fraction=float(fl[0]), open_fraction=float(fl[1]), poly_fraction=float(fl[2]),
                    v_mean=float(v), eta_mean=float(eta), faces_mean=float(faces),
                    v_variance=float(obs.volume_fluctuation(o["sums"].sum(0))),
                    largest_face_sides=int(np.flatnonzero(o["side_hist"])[-1]))
    res.update(full_over_shell=med["full_7.0"] / med["shell"], full_7_5_over_shell=med["full_7.5"] / med["shell"],
               hists_over_shell=med["hists"] / med["shell"], flags_over_shell=med["flags"] / med["shell"],
               lists_share_of_full=med["lists"] / med["full_7.0"], no_prune_over_full=med["no_prune"] / med["full_7.0"],
               cells_per_s=R * n / (med["full_7.0"] * 1e-3), frame_7_0=frame(vo), frame_7_5=frame(out["full_7.5"]))
    if "details" in sides:
        res["details_over_full"] = med["details"] / med["full_7.0"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", default="4096,61440")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--details-max", type=int, default=4096,
                    help="largest R at which the per-molecule outputs are timed (1 KiB a molecule on the host, twice)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    a = mio.load_nist_fixture(4, "unwrapped")
    res = {"bench": "voronoi", "system": "SPC/E, NIST configuration 4",
           "sizes": [one_size(a, int(r), args.rounds, args.details_max) for r in args.replicas.split(",")]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
