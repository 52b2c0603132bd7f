#!/usr/bin/env python3
"""Widom insertion of solute pairs (mmc_batch_widom_pair) against what a user could compose before it
existed, on one GPU, one process: 750-molecule SPC/E (NIST config 4) at R = 4096 and at bench.py's
headline replica count, M = 64 insertions per replica and call, K = 16 separations.  Two pairs:
methane-methane (uncharged instantiation) and water-water (charged).

Per size and pair, after a warm-up of every side, --rounds rounds of, in turn,
  (a) one widom_pair call: the sums of g_AB(d) at all K separations;
  (b) the composition: one widom_solute call for A with its placements and terms downloaded, then
      per separation B's placements made on the host (one random ray and rotation per insertion,
      drawn before the clock starts), uploaded through widom_solute_at, its terms downloaded, the
      A-B term added on the host (LJ, and for charges the real-space erfc term; the reciprocal
      cross term is LEFT OUT of (b), which only makes (b) cheaper) and the weights exponentiated
      and summed there: K + 1 launches and drains;
  (c) one widom_solute(M) call of the same solute without outputs: (a) / ((K + 1) (c)) shows what
      the shared neighbourhood of the K + 1 placements bought over K + 1 independent insertions.
Every call returns after the device is done and the sums are on the host.  The JSON has every
sample, medians and the spread, the ratios of the medians and the pair-insertions/s
(R M K / median of (a)); nothing is enforced.

    python3 scripts/solute_pair_bench.py [--replicas 4096,61440] [--rounds 3] [--out profiles/solute_pair_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
from scipy.special import erfc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metropolismontecarlo_amd import io as mio, structs  # noqa: E402
from metropolismontecarlo_amd.device import Batch  # noqa: E402

T, DR, DPHI, RCUT = 298.15, 0.316555789, 0.05, 10.0
M, K = 64, 16


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    return {"ms": ms, "median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def pairs(a, offsets):
    st = np.asarray(a["atype"][:3]) - 1
    e_w, s_w = np.diag(a["eps"])[st], np.diag(a["sig"])[st]
    water = structs.Solute("water", offsets, a["charge"][:3], a["eps"][st][:, st], a["sig"][st][:, st])
    methane = structs.Solute("methane", np.zeros((1, 3)), [0.0], np.sqrt(147.9 * e_w)[None, :],
                             ((3.73 + s_w) / 2)[None, :])
    return (structs.SolutePair(methane, methane, [[147.9]], [[3.73]]),
            structs.SolutePair(water, water, a["eps"][st][:, st], a["sig"][st][:, st]))


def image(d, box):
    return d - box * np.round(d / box)


def host_cross(pair, mol_a, mol_b, box, kappa):
    """The A-B term of one separation on the host, (R, M): LJ and real-space Coulomb under the COM
    gates (the reciprocal cross term is left out)."""
    SA, SB = pair.a.n_sites, pair.b.n_sites
    c2 = (image(mol_b[:, :, SB] - mol_a[:, :, SA], box) ** 2).sum(-1)
    gate = c2 < RCUT * RCUT
    x = np.zeros(c2.shape)
    for i in range(SA):
        for j in range(SB):
            r2 = (image(mol_b[:, :, j] - mol_a[:, :, i], box) ** 2).sum(-1)
            if pair.eps_ab[i, j] > 0.001:
                s6 = (pair.sig_ab[i, j] ** 2 / r2) ** 3
                x += 4 * pair.eps_ab[i, j] * (s6 * s6 - s6)
            qq = pair.a.charge[i] * pair.b.charge[j]
            if qq != 0.0:
                r = np.sqrt(r2)
                x += structs.factor * qq * erfc(kappa * r) / r
    return np.where(gate, x, 0.0)


def composition(b, pair, d, frames, seed):
    """(b): boltz_ab (R, K) from one widom_solute call, K widom_solute_at calls and the host."""
    box, kappa = b.box, 5.6 / b.box
    nh, rb = frames
    bs_a, _, mol_a, du_a, ov_a = b.widom_solute(pair.a, M, T, seed=seed, outputs=True)
    u_a = du_a.sum(-1)
    out = np.zeros((b.R, len(d)))
    for k, dk in enumerate(d):
        cb = (mol_a[:, :, -1] + dk * nh) % box
        mol_b = np.concatenate([cb[:, :, None] + rb, cb[:, :, None]], axis=2)
        _, _, du_b, ov_b = b.widom_solute_at(pair.b, mol_b, T)
        u = u_a + du_b.sum(-1) + host_cross(pair, mol_a, mol_b, box, kappa)
        with np.errstate(over="ignore", invalid="ignore"):
            w = np.where((ov_a != 0) | (ov_b != 0), 0.0, np.exp(-u / T))
        out[:, k] = w.sum(1)
    return bs_a, out


def one_size(a, R, rounds):
    box = float(a["box"])
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], box, 5.6 / box,
              structs.factor, RCUT, RCUT)
    b.set_option("device_moves", 1)
    e = b.potential_ewald(as_array=True)["energy"].copy()
    e, _ = b.run(64, T, DR, DPHI, seed=11, energies=e, n_groups=2, n_threads=1)   # replicas diverge
    d = np.linspace(3.0, 0.49 * box, K)
    rng = np.random.default_rng(17)
    res = {"replicas": R, "n_mol": int(a["com"].shape[0]), "n_insert": M, "n_sep": K, "d": d.tolist()}
    for pair in pairs(a, b.widom_offsets):
        name = pair.a.name
        # the host's rays and orientations of B, one per insertion (drawn before the clock starts)
        nh = rng.normal(size=(R, M, 3))
        nh /= np.linalg.norm(nh, axis=-1, keepdims=True)
        q = rng.normal(size=(R, M, 4))
        q /= np.linalg.norm(q, axis=-1, keepdims=True)
        w, x, y, z = (q[..., i] for i in range(4))
        rot = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                        np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                        np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)
        rb = np.einsum("rmde,se->rmsd", rot, pair.b.offsets)
        sides = [("pair", lambda: b.widom_pair(pair, d, M, T, seed=5)),
                 ("composition", lambda: composition(b, pair, d, (nh, rb), 5)),
                 ("solute", lambda: b.widom_solute(pair.a, M, T, seed=5))]
        out = {}
        for nm, fn in sides:                # warm-up: code load, first allocations
            out[nm] = fn()
        # all three insert the same A: the same single-solute sums to rounding
        ref = out["solute"][0]
        assert np.all(np.abs(out["pair"]["boltz_a"] - ref) <= 1e-9 * np.abs(ref) + 1e-300)
        assert np.all(np.abs(out["composition"][0] - ref) <= 1e-9 * np.abs(ref) + 1e-300)
        ms = {nm: [] for nm, _ in sides}
        for _ in range(rounds):
            for nm, fn in sides:
                ms[nm].append(timed(fn)[0])
        r = {nm: summary(ms[nm]) for nm, _ in sides}
        med = {nm: r[nm]["median_ms"] for nm, _ in sides}
        r["sites"] = [pair.a.n_sites, pair.b.n_sites]
        r["pair_insertions_per_s"] = R * M * K / (med["pair"] * 1e-3)
        r["pair_over_composition_median"] = med["pair"] / med["composition"]
        r["pair_over_k_plus_1_solute_calls_median"] = med["pair"] / ((K + 1) * med["solute"])
        res[name + "_" + pair.b.name] = r
        print(f"R = {R} {name}-{pair.b.name}: {med}", file=sys.stderr, flush=True)
    b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", default="4096,61440")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    a = mio.load_nist_fixture(4, "unwrapped")
    res = {"bench": "solute_pair", "system": "SPC/E, NIST configuration 4", "sizes": []}
    for r in args.replicas.split(","):
        res["sizes"].append(one_size(a, int(r), args.rounds))
        line = json.dumps(res)
        if args.out:                        # (kept after every size)
            with open(args.out, "w") as fh:
                fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
