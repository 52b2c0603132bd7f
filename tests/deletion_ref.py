"""Restatements for the deletion-energy tests (mmc_batch_deletion, include/mmc_hip.h): the oracle's
terms of one existing molecule, the binning rule in numpy and the fixed-order sums of
k_deletion_reduce on the host.  Not a test module."""
import numpy as np

import common


def without(a, com, coords, i):
    """(com, coords) of the configuration with molecule i (0-based) taken out."""
    com, coords = np.asarray(com, dtype=float), np.asarray(coords, dtype=float)
    keep = np.ones(com.shape[0], dtype=bool)
    keep[i] = False
    return com[keep], coords[np.repeat(keep, 3)]


def record(com, coords, i):
    """Molecule i as a Widom test molecule: atoms (9) then COM (3)."""
    return np.concatenate([np.asarray(coords)[3 * i:3 * i + 3].ravel(), np.asarray(com)[i]])


def oracle_terms(orc, a, com, coords, i, box, lj_rcut, qq_rcut, alpha=5.6):
    """(d_lj, d_real, d_recip, overlap) of molecule i (0-based) of the configuration (com, coords) of
    the system `a` (topology and tables: identical 3-atom molecules) in the box `box`,
    kappa = alpha / box.  dU is what potential(..., "ewald") loses when the molecule is taken out:
      d_lj    == orc.lj_poly_du(i)
      d_real  == orc.ewald_short(i)                      (0 when it reports an overlap)
      d_recip == factor (recip_long(N) - recip_long(N \\ i)) + orc.ewald_self(the molecule's charges)
    The self term is taken directly, not by cancelling two 1e7 K numbers (common.widom_oracle_terms
    does the same); RecipLong is recomputed from the coordinates, so a wrong S buffer shows."""
    from metropolismontecarlo_amd import structs
    com, coords = np.asarray(com, dtype=float), np.asarray(coords, dtype=float)
    n, L = com.shape[0], float(box)
    first = np.arange(1, 3 * n, 3, dtype=np.int64)
    q = np.asarray(a["charge"][:3 * n], dtype=float)
    s = orc.System(com, first, first + 2, coords, np.asarray(a["atype"])[:3 * n], q, a["eps"], a["sig"], L)
    ew = orc.Ewald(alpha / L, 5, 27, L, factor=structs.factor)
    lj, _ = orc.lj_poly_du(i + 1, s, lj_rcut)
    real, _, ov = orc.ewald_short(i + 1, s, ew, qq_rcut)
    _, rest = without(a, com, coords, i)
    rl1 = orc.recip_long(ew, coords, q, L)
    rl0 = orc.recip_long(ew, rest, q[:3 * (n - 1)], L)
    recip = ew.factor * (rl1 - rl0) + orc.ewald_self(ew, q[3 * i:3 * i + 3])
    return lj, real, recip, ov


def check(orc, a, b, r, sel, du, ovl, lj_rcut, qq_rcut, alpha=5.6, what=""):
    """Every term and the overlap flag of replica r's selected molecules sel [n] (rows du [n, 3],
    ovl [n]) against the oracle, on the replica's own coordinates and box.  Tolerance per term:
    common.widom_close (1e-9 K + 1e-13 of the term)."""
    com, coords, _ = b.get_replica(r)
    box = float(b.get_boxes()[r])
    bad = []
    for k, i in enumerate(sel):
        lj, real, recip, ov = oracle_terms(orc, a, com, coords, int(i), box, lj_rcut, qq_rcut, alpha)
        if bool(ovl[k] & 1) != ov:
            bad.append((int(i), "overlap", int(ovl[k]), ov))
        for name, x, ref in (("lj", du[k, 0], lj), ("real", du[k, 1], real), ("recip", du[k, 2], recip)):
            if not common.widom_close(x, ref):
                bad.append((int(i), name, x, ref))
    assert not bad, f"{what} replica {r}: {bad[:6]}"


def energy_bins(du, n_bins, u_lo, u_hi):
    """Slots [n_bins + 2] of the values du, the header's rule restated independently of
    observables.energy_bins: s = n_bins / (u_hi - u_lo); below u_lo slot 0; at or above u_hi, or
    floor((dU - u_lo) * s) >= n_bins, slot n_bins + 1; else floor((dU - u_lo) * s) + 1.  NaN is in
    no slot."""
    s = np.float64(n_bins) / (np.float64(u_hi) - np.float64(u_lo))
    h = np.zeros(n_bins + 2, dtype=np.uint64)
    for x in np.asarray(du, dtype=np.float64).ravel():
        if x != x:
            continue
        if x < u_lo:
            h[0] += 1
        elif x >= u_hi:
            h[n_bins + 1] += 1
        else:
            k = np.floor((x - np.float64(u_lo)) * s)
            h[n_bins + 1 if k >= n_bins else int(k) + 1] += 1
    return h


def wave_sum_rows(v):
    """csrc/mmc_device.hpp wave_sum_rows on 64 lane values: an inclusive scan inside each row of 16
    lanes by shifts of 1, 2, 4, 8 (a lane without a partner adds 0.0), then the four row totals
    ((r0 + r1) + r2) + r3."""
    v = np.array(v, dtype=np.float64).reshape(4, 16)
    for sh in (1, 2, 4, 8):
        moved = np.zeros_like(v)
        moved[:, sh:] = v[:, :-sh]
        v = v + moved
    r = v[:, 15]
    return ((r[0] + r[1]) + r[2]) + r[3]


def host_sums(du, ovl, temperature, boltz0=None, nflag0=None):
    """k_deletion_reduce on the host, from the returned rows du [R, n, 3] and flags ovl [R, n]:
    lane l adds the replica's unflagged entries l, l + 64, ... in that order (three terms, 1.0 and
    exp(dU * (1 / T)), dU = (d_lj + d_real) + d_recip), the 64 lane sums go through wave_sum_rows,
    boltz0 is added last.  Returns (esum [R, 4], boltz [R], n_flagged [R])."""
    du, ovl = np.asarray(du, dtype=np.float64), np.asarray(ovl)
    R, n = ovl.shape
    esum, boltz = np.zeros((R, 4)), np.zeros(R)
    nfl = np.zeros(R, dtype=np.int64) if nflag0 is None else np.array(nflag0, dtype=np.int64).copy()
    inv_t = 1.0 / temperature
    for r in range(R):
        acc = np.zeros((5, 64))
        for e in range(n):
            if ovl[r, e]:
                continue
            t = du[r, e]
            d = (t[0] + t[1]) + t[2]
            lane = e % 64
            acc[0, lane] += t[0]
            acc[1, lane] += t[1]
            acc[2, lane] += t[2]
            acc[3, lane] += 1.0
            acc[4, lane] += np.exp(d * inv_t)
        for q in range(4):
            esum[r, q] = wave_sum_rows(acc[q])
        boltz[r] = (0.0 if boltz0 is None else boltz0[r]) + wave_sum_rows(acc[4])
        nfl[r] += int(np.count_nonzero(ovl[r]))
    return esum, boltz, nfl
