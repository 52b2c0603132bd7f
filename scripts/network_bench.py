#!/usr/bin/env python3
"""One hbond_network call (clusters and percolation of the hydrogen-bond graph,
mmc_batch_hbond_network) with one criterion and with eight, against one local_order(400) call, on
one GPU, one process: 750-molecule SPC/E (NIST config 4) at bench.py's headline replica count.

After a warm-up of all sides, --rounds rounds of
  (a1) one hbond_network call with the criterion (3.5 A, 30 degrees, 0), summed histograms and the
       per-replica stats: N (N - 1) O-O distances per replica, both directions of every candidate
       pair, then the label propagation of 750 sites in LDS;
  (a8) the same with eight criteria, r_hb = 2.9 .. 3.6 A at 30 degrees: two passes over the molecules
       with four criteria each (what one workgroup's LDS holds lists of), eight cluster phases;
  (a0) (a1) with min_bonds = 16: the same bonds, but no molecule is a site, so the cluster phase is
       its fixed part and one round: what the bond phase costs;
  (b)  one local_order(400) call, summed output: the same O(N^2) oxygen scan,
taken in turn (a1, a8, a0, b, a1, ...) so that drift hits all alike.  Every call is synchronous: it
returns after the device is done and the output is on the host.  The JSON has every sample, medians
and the spread (min, max), the ratios a1 / b and a8 / (8 a1), and the number of propagation rounds
of a sample of replicas: the rounds are not an output of the call, so the sample's partner lists
(details=True on a small batch of the same configurations) are propagated on the host by the
kernel's own rule, min over the bonded sites until a round changes nothing.  No ratio is a bar.

    python3 scripts/network_bench.py [--replicas 61440] [--rounds 7] [--out profiles/network_bench.json]
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
Q_BINS = 400
R_HB8 = (2.9, 3.0, 3.1, 3.2, 3.3, 3.4, 3.5, 3.6)
SAMPLE = 32


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    return {"ms": ms, "median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def host_rounds(label, nbr):
    """Rounds of synchronous min-label propagation over the sites (label >= 0) of one replica and
    criterion, the last, which changes nothing, included."""
    n = label.shape[0]
    big = n
    site = label >= 0
    lab = np.where(site, np.arange(n), big)
    idx = np.where(nbr >= 0, nbr, 0)
    rounds = 0
    while True:
        rounds += 1
        nb = np.where(nbr >= 0, lab[idx], big).min(1)
        new = np.where(site, np.minimum(lab, nb), big)
        if np.array_equal(new, lab):
            assert np.array_equal(np.where(site, lab, -1), label)
            return rounds
        lab = new


def sample_rounds(a, b, crit):
    """Propagation rounds per (replica, criterion) of SAMPLE replicas spread over the batch."""
    box = float(a["box"])
    pick = np.linspace(0, b.R - 1, min(SAMPLE, b.R)).astype(int)
    s = Batch(len(pick), a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, 5.6 / box,
              structs.factor, RCUT, RCUT)
    for k, r in enumerate(pick):
        rep = b.get_replica(int(r))
        s.set_replica(k, rep[0], rep[1])
    out = s.hbond_network(crit, 30.0, 0, per_replica=True, details=True)
    s.close()
    return np.array([[host_rounds(out["label"][r, k], out["nbr"][r, k]) for k in range(len(crit))]
                     for r in range(len(pick))])


def one_size(a, R, rounds):
    box = float(a["box"])
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, 5.6 / box,
              structs.factor, RCUT, RCUT)
    b.set_option("device_moves", 1)
    e = b.potential_ewald(as_array=True)["energy"].copy()
    e, _ = b.run(64, T, DR, DPHI, seed=11, energies=e, n_groups=2, n_threads=1)   # replicas diverge

    sides = {"hbond_network_1": lambda: b.hbond_network(3.5, 30.0, 0),
             "hbond_network_8": lambda: b.hbond_network(R_HB8, 30.0, 0),
             "hbond_network_1_no_sites": lambda: b.hbond_network(3.5, 30.0, 16),
             "local_order": lambda: b.local_order(Q_BINS)}
    for _ in range(2):                      # warm-up: code load, first allocations, the LDS opt-in
        out = {k: f() for k, f in sides.items()}
    n = a["com"].shape[0]
    st1, st8 = out["hbond_network_1"]["stats"], out["hbond_network_8"]["stats"]
    assert np.array_equal(st1[:, 0], st8[:, 6]) and int(st8[..., 7].sum()) == 0
    st0 = out["hbond_network_1_no_sites"]["stats"]
    assert np.array_equal(st0[:, 0, 0], st1[:, 0, 0]) and int(st0[:, 0, 1:].sum()) == 0
    assert np.all(out["hbond_network_8"]["size_hist"] @ np.arange(n + 1, dtype=np.uint64) == n * R)
    ms = {k: [] for k in sides}
    for _ in range(rounds):
        for k, f in sides.items():
            ms[k].append(timed(f)[0])
    rnd = sample_rounds(a, b, R_HB8)
    b.close()
    res = {"replicas": R, "n_mol": int(n), "r_hb_1": 3.5, "r_hb_8": list(R_HB8), "theta_deg": 30.0, "q_bins": Q_BINS}
    res.update({k: summary(v) for k, v in ms.items()})
    res["one_over_local_order"] = res["hbond_network_1"]["median_ms"] / res["local_order"]["median_ms"]
    res["eight_over_eight_ones"] = res["hbond_network_8"]["median_ms"] / (8.0 * res["hbond_network_1"]["median_ms"])
    res["bond_phase_share_of_one"] = res["hbond_network_1_no_sites"]["median_ms"] / res["hbond_network_1"]["median_ms"]
    res["oo_distances_per_s_1"] = n * (n - 1) * R / (res["hbond_network_1"]["median_ms"] * 1e-3)
    res["propagation_rounds"] = {"replicas_sampled": int(rnd.shape[0]),
                                 "how": "host propagation of the sample's partner lists, final unchanged round included",
                                 "mean_by_r_hb": [float(x) for x in rnd.mean(0)],
                                 "max_by_r_hb": [int(x) for x in rnd.max(0)]}
    res["wrapping_fraction_by_r_hb"] = [float(x) for x in (st8[..., 5] != 0).mean(0)]
    res["bonds_per_molecule_by_r_hb"] = [float(x) for x in 2.0 * st8[..., 0].mean(0) / n]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", default="61440")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    a = mio.load_nist_fixture(4, "unwrapped")
    res = {"bench": "hbond_network", "system": "SPC/E, NIST configuration 4",
           "sizes": [one_size(a, int(r), args.rounds) for r in args.replicas.split(",")]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
