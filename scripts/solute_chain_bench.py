#!/usr/bin/env python3
"""What a fixed solute costs a run at bench.py's headline shape.

    python scripts/solute_chain_bench.py [--repeats 3] [--out profiles/solute_chain_bench.json]

61440 chains of NIST configuration 4 (750 molecules), moves drawn on the device, calls of 20 and of
600 steps with bench.py's constants; bench.py itself is not touched.  Each repeat is a fresh child
process per variant, the variants taken in turn, all of the same build:
  (a) default:  no solute, the path the library chooses (the kernel decides, several steps a launch),
  (b) host:     no solute, accept_on_device = 0 and steps_per_launch = 1 -- the path a solute forces:
                the host decides, a launch per step,
  (c) methane:  (b)'s path with one uncharged LJ site set in the largest cavity of the configuration,
  (d) charged3: (b)'s path with a three-site charged solute (the batch's own molecule as a foreign
                solute: SPC/E's charges and LJ rows) in the same cavity.
Per variant and call length: moves/s over the timed calls, and the mean span of a launch between the
HIP events that bracket it (mmc_run_stats::kernel_ms / timed_launches, every 8th launch): with a
solute the bracket holds k_solute_move and the move kernel behind it, so (c) - (b) and (d) - (b) of
that span is what k_solute_move adds to a launch.  Recorded, not gated.  Writes one JSON object.

    python scripts/solute_chain_bench.py --observables [--out profiles/solute_observables_bench.json]

times, in one process, the two observables of a solute on the same batch (no moves): the wall time of
Batch.solute_energy and of Batch.rdf_solute(200 bins to 10 A, summed over the replicas), five calls
each after one untimed, for methane and for a 16-site solute (SPC/E's oxygen row on every site,
charges +-0.1) in the same cavity.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODES = ("default", "host", "methane", "charged3")
CALLS = {20: 20, 600: 2}     # timed calls per call length


def cavity(a, n_try=4000, seed=1):
    """The candidate point (of n_try uniform ones) farthest from every atom, by the minimum image."""
    import numpy as np
    box = float(a["box"])
    pts = np.random.default_rng(seed).random((n_try, 3)) * box
    best, best_d = None, -1.0
    for k0 in range(0, n_try, 500):
        d = pts[k0:k0 + 500, None, :] - np.asarray(a["coords"])[None, :, :]
        d -= box * np.round(d / box)
        m = np.sqrt((d * d).sum(2)).min(1)
        if m.max() > best_d:
            best, best_d = pts[k0 + int(m.argmax())], float(m.max())
    return best, best_d


def solute_for(mode, a):
    """(structs.Solute, mol [S + 1][3]) of a variant, or None."""
    import numpy as np
    from metropolismontecarlo_amd import structs
    if mode in ("default", "host"):
        return None
    c, _ = cavity(a)
    st = np.asarray(a["atype"][:3]) - 1
    eps, sig = np.asarray(a["eps"]), np.asarray(a["sig"])
    if mode == "methane":        # OPLS united atom against the water slots, Lorentz-Berthelot
        e_w, s_w = np.diag(eps)[st], np.diag(sig)[st]
        sol = structs.Solute("methane", np.zeros((1, 3)), [0.0], np.sqrt(147.9 * e_w)[None, :], ((3.73 + s_w) / 2)[None, :])
    else:
        off = np.asarray(a["coords"][:3]) - np.asarray(a["com"][0])
        off -= a["box"] * np.round(off / a["box"])
        sol = structs.Solute("water", off, np.asarray(a["charge"][:3]), eps[st][:, st], sig[st][:, st])
    return sol, np.vstack([c + sol.offsets, c])


def one(mode, replicas, warmup_calls, threads):
    """One measurement in this process: prints a JSON line."""
    import numpy as np
    import bench
    from metropolismontecarlo_amd import io as mio
    from metropolismontecarlo_amd import sharding, structs
    from metropolismontecarlo_amd.device import Batch
    a = mio.load_nist_fixture(4, "unwrapped")
    box = a["box"]
    b = Batch(replicas, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, 5.6 / box,
              structs.factor, bench.RCUT, bench.RCUT)
    b.set_option("device_moves", 1)
    if mode != "default":
        b.set_option("accept_on_device", 0)
        b.set_option("steps_per_launch", 1)
    sol = solute_for(mode, a)
    if sol is not None:
        b.set_solute(*sol)
    energies = b.potential_ewald(as_array=True)["energy"].copy()
    kw = dict(n_groups=2, n_threads=threads, time_kernels=8)
    T, dr, dphi = bench.TEMPERATURE, bench.DR_MAX, bench.DPHI_MAX
    out = {"mode": mode, "sites": 0 if sol is None else sol[0].n_sites, "calls": {}}
    for _ in range(warmup_calls):
        energies, _ = b.run(20, T, dr, dphi, sharding.run_seed(phase=0), energies, **kw)
    for steps, calls in CALLS.items():
        n_moves = n_dev = launches = 0
        k_ms = 0.0
        t0 = time.perf_counter()
        for _ in range(calls):
            energies, st = b.run(steps, T, dr, dphi, sharding.run_seed(phase=1), energies, **kw)  # (returns synchronised)
            n_moves += st["moves"]
            n_dev += st["device_decisions"]
            k_ms += st["kernel_ms"]
            launches += st["timed_launches"]
        elapsed = time.perf_counter() - t0
        out["calls"][str(steps)] = {"moves_per_s": n_moves / elapsed, "elapsed_s": elapsed, "moves": n_moves,
                                    "device_decisions": n_dev, "timed_launches": launches,
                                    "launch_span_us": 1e3 * k_ms / max(launches, 1)}
    tot = b.potential_ewald(as_array=True)
    out["energy_drift_rel"] = float(np.max(np.abs(energies - tot["energy"]) / np.abs(energies)))
    out["n_overlap"] = int(tot["n_overlap"].sum())
    if sol is not None:
        u_lj, u_real, _ = b.solute_energy()
        out["u_sw_mean"] = float((u_lj + u_real).mean())
    b.close()
    print(json.dumps(out))


def observables(replicas, out_path):
    import numpy as np
    import bench
    from metropolismontecarlo_amd import io as mio
    from metropolismontecarlo_amd import structs
    from metropolismontecarlo_amd.device import Batch
    a = mio.load_nist_fixture(4, "unwrapped")
    box = a["box"]
    b = Batch(replicas, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, 5.6 / box,
              structs.factor, bench.RCUT, bench.RCUT)
    c, _ = cavity(a)
    st = np.asarray(a["atype"][:3]) - 1
    rng = np.random.default_rng(2)
    off = rng.normal(size=(16, 3)) * 0.8
    big = structs.Solute("sites16", off, np.tile([0.1, -0.1], 8), np.tile(np.asarray(a["eps"])[st][:1, st], (16, 1)),
                         np.tile(np.asarray(a["sig"])[st][:1, st], (16, 1)))
    res = {"shape": {"replicas": replicas, "system": "NIST SPC/E configuration 4 (750 molecules)", "numbins": 200,
                     "r_max": 10.0, "per_replica": 0, "timed_calls": 5}, "gated": False, "results": {}}
    for sol, mol in (solute_for("methane", a), (big, np.vstack([c + big.offsets, c]))):
        b.set_solute(sol, mol)
        b.recip_long()
        t = {"solute_energy_ms": [], "rdf_solute_ms": []}
        for k in range(6):
            t0 = time.perf_counter()
            b.solute_energy()
            t1 = time.perf_counter()
            h = b.rdf_solute(200, 10.0)
            t2 = time.perf_counter()
            if k:
                t["solute_energy_ms"].append(1e3 * (t1 - t0))
                t["rdf_solute_ms"].append(1e3 * (t2 - t1))
        res["results"][sol.name] = {"sites": sol.n_sites, "counted_distances": int(h.sum()),
                                    **{k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in t.items()}}
    b.close()
    text = json.dumps(res, indent=1)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--observables", action="store_true")
    ap.add_argument("--one", choices=MODES)
    ap.add_argument("--replicas", type=int, default=61440)
    ap.add_argument("--warmup-calls", type=int, default=6)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=150, help="seconds per child process")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.observables:
        observables(args.replicas, args.out)
        return 0
    if args.one:
        one(args.one, args.replicas, args.warmup_calls, args.threads)
        return 0
    res = {m: [] for m in MODES}

    def report():
        out = {"shape": {"replicas": args.replicas, "system": "NIST SPC/E configuration 4 (750 molecules)",
                         "timed_calls": {str(k): v for k, v in CALLS.items()}, "warmup_calls_of_20": args.warmup_calls,
                         "host_threads": args.threads, "groups": 2, "device_moves": 1},
               "gated": False, "results": {}}
        for m in MODES:
            if not res[m]:
                continue
            out["results"][m] = {"repeats": res[m]}
            for steps in CALLS:
                v = [r["calls"][str(steps)]["moves_per_s"] for r in res[m]]
                s = [r["calls"][str(steps)]["launch_span_us"] for r in res[m]]
                out["results"][m][str(steps)] = {"moves_per_s_median": statistics.median(v), "moves_per_s_min": min(v),
                                                 "moves_per_s_max": max(v), "launch_span_us_median": statistics.median(s)}
        if all(res.values()):
            for steps in CALLS:
                k = str(steps)
                host = out["results"]["host"][k]
                for m in ("methane", "charged3"):
                    out[f"{m}_time_over_host_{k}"] = host["moves_per_s_median"] / out["results"][m][k]["moves_per_s_median"]
                    out[f"{m}_k_solute_move_us_per_launch_{k}"] = (out["results"][m][k]["launch_span_us_median"]
                                                                   - host["launch_span_us_median"])
                out[f"host_time_over_default_{k}"] = (out["results"]["default"][k]["moves_per_s_median"]
                                                      / host["moves_per_s_median"])
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
        return out

    out = {}
    for rep in range(args.repeats):
        for mode in MODES:               # in turn within a repeat: drift of the machine hits all alike
            cmd = [sys.executable, os.path.abspath(__file__), "--one", mode, "--replicas", str(args.replicas),
                   "--warmup-calls", str(args.warmup_calls), "--threads", str(args.threads)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            if p.returncode != 0:        # nothing more is started on the GPU after a failure
                sys.stderr.write(p.stdout + p.stderr)
                print(f"{mode} repeat {rep}: exit status {p.returncode}; stopping", file=sys.stderr)
                return 1
            r = json.loads(p.stdout.strip().splitlines()[-1])
            res[mode].append(r)
            print(f"{mode} #{rep}: " + ", ".join(f"{k} steps {v['moves_per_s']:.4g} moves/s" for k, v in r["calls"].items()),
                  flush=True)
        out = report()                   # after every repeat: a session cut short keeps its full repeats
    print(json.dumps({k: v for k, v in out.items() if k not in ("shape", "results")}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
