"""Helpers of the solute-pair tests (test_solute_pair_abi.py, test_solute_pair_host.py,
test_gpu_solute_pair.py, test_solute_paths_host.py, test_gpu_solute_paths.py): the pairs the tests
insert and the oracle's statement of every term --
solute_ref.SoluteOracle for A alone and for B alone on N + 1 molecules, and for the A-B term x the
oracle's lj_poly_du(2), ewald_short(2) and factor (recip_long(A u B) - recip_long(A) - recip_long(B))
on a System that holds only A and B in the same box, with eps_ab / sig_ab as its type table."""
import os
import re

import numpy as np

import common
import solute_ref as sr
from metropolismontecarlo_amd import structs

T = sr.T
RCUT = 10.0
# test_gpu_solute_pair.py's shapes and the draws of its multi-site case (precondition in
# test_solute_pair_host.py: among these the oracle alone sets some flags and leaves others unset)
R, M = 8, 8
MULTI_SEED, MULTI_DRAW0 = 83, 2
MULTI_D = (2.0, 3.5, 6.0, 11.0)
# |sum of terms - difference of totals| / max |total|, the largest test_solute_pair_host.py finds
WHOLE_CANCELLATION = 1.1e-15
HPP = os.path.join(common.HERE, "..", "metropolismontecarlo_amd", "csrc", "mmc_solute_pair.hpp")


# ---- pairs ------------------------------------------------------------------------------------------
def cross(eps_a, sig_a, eps_b, sig_b):
    """eps_ab / sig_ab (S_A, S_B) by the reference's mixing from the sites' own parameters."""
    ea, sa, eb, sb = (np.asarray(x, dtype=float) for x in (eps_a, sig_a, eps_b, sig_b))
    return np.sqrt(ea[:, None] * eb[None, :]), (sa[:, None] + sb[None, :]) / 2


def methane_pair(a):
    """Two united-atom methanes (OPLS-UA 147.9 K, 3.73 A): uncharged."""
    m = sr.methane(a)
    return structs.SolutePair(m, m, *cross([147.9], [3.73], [147.9], [3.73]))


def anion(a):
    """A single site with q = -1 (chloride-like LJ: 50.3 K, 4.4 A)."""
    eps, sig = sr.mixed_rows(a, [50.3], [4.4])
    return structs.Solute("anion", np.zeros((1, 3)), [-1.0], eps, sig)


def ion_pair(a):
    return structs.SolutePair(sr.cation(a), anion(a), *cross([65.4], [2.35], [50.3], [4.4]))


def synthetic_pair(a, SA=5, SB=11):
    """solute_ref.synthetic(SA) with synthetic(SB); a cross table of its own with every fourth
    entry without LJ."""
    A, B = sr.synthetic(a, SA, seed=SA), sr.synthetic(a, SB, seed=SB)
    rng = np.random.default_rng(100 * SA + SB)
    eps = 30.0 + 70.0 * rng.random((SA, SB))
    eps.ravel()[3::4] = 0.0
    return structs.SolutePair(A, B, eps, 2.5 + rng.random((SA, SB)))


def water_dipole_pair(a, offsets):
    """The batch's own molecule as A, solute_ref.dipole as B."""
    st = sr.slot_types(a) - 1
    e_w, s_w = np.diag(np.asarray(a["eps"]))[st], np.diag(np.asarray(a["sig"]))[st]
    return structs.SolutePair(sr.water_solute(a, offsets), sr.dipole(a), *cross(e_w, s_w, [110.0, 0.0], [3.4, 0.0]))


def water_pair(a, offsets):
    st = sr.slot_types(a) - 1
    w = sr.water_solute(a, offsets)
    return structs.SolutePair(w, w, np.asarray(a["eps"])[st][:, st], np.asarray(a["sig"])[st][:, st])


def ghost(S=1):
    """A solute that interacts with nothing."""
    return structs.Solute("ghost", np.zeros((S, 3)), np.zeros(S), np.zeros((S, 3)), np.zeros((S, 3)))


def water_offsets(a):
    return np.asarray(a["coords"][:3], dtype=float) - np.asarray(a["com"][0], dtype=float)


# ---- the kernel's scan, from its own constants --------------------------------------------------------
def kernel_constants():
    src = open(HPP).read()
    hsol = open(os.path.join(os.path.dirname(HPP), "mmc_solute.hpp")).read()
    tile = int(re.search(r"#define PAIR_TILE (\d+)", src).group(1))
    n_list = int(re.search(r"#define SOL_LIST (\d+)", hsol).group(1))
    assert "base += 256" in src and "SOL_LIST - 256" in src and "p0 += PAIR_TILE" in src
    return tile, n_list


def tile_scans_flush(com, c_a, c_b, gate, box):
    """Whether EVERY tile of k_solute_pair_wave's pair part (mmc_solute_pair.hpp) certainly empties
    its neighbour list mid-scan and has neighbours left for a later process() call.  The placements
    (A, B_0, B_1, ...) are taken PAIR_TILE at a time; a tile's scan lists the waters the 16-bit
    prefilter of ANY of its placements admits, in trips of 256, and empties the list after a trip
    when it holds more than SOL_LIST - 256 entries.  Counted is the union of the exact gates by a
    relative margin of 1e-9 -- a lower bound on the prefilters' union (solute_ref.scan_flushes'
    argument)."""
    tile, n_list = kernel_constants()
    com = np.asarray(com, dtype=float)
    centres = [np.asarray(c_a, dtype=float)] + [np.asarray(c, dtype=float) for c in c_b]
    for p0 in range(0, len(centres), tile):
        gated = np.zeros(com.shape[0], dtype=bool)
        for c in centres[p0:p0 + tile]:
            d = com - c
            d = d + common.image_shift(d, box)
            gated |= (d * d).sum(1) < gate * gate * (1 - 1e-9)
        before = np.cumsum(gated)
        if not any(before[b - 1] > n_list - 256 and before[-1] - before[b - 1] > 0
                   for b in range(256, gated.shape[0], 256)):
            return False
    return True


# ---- the oracle -------------------------------------------------------------------------------------
class PairOracle:
    def __init__(self, orc, a, pair, lj_rcut=RCUT, qq_rcut=RCUT, alpha=5.6):
        self.orc, self.a, self.pair = orc, a, pair
        self.lj_rcut, self.qq_rcut, self.alpha = lj_rcut, qq_rcut, alpha
        self.oa = sr.SoluteOracle(orc, a, pair.a, lj_rcut, qq_rcut, alpha)
        self.ob = sr.SoluteOracle(orc, a, pair.b, lj_rcut, qq_rcut, alpha)
        SA, SB = pair.a.n_sites, pair.b.n_sites
        self.eps = np.zeros((SA + SB, SA + SB))
        self.sig = np.zeros((SA + SB, SA + SB))
        self.eps[:SA, SA:], self.eps[SA:, :SA] = pair.eps_ab, pair.eps_ab.T
        self.sig[:SA, SA:], self.sig[SA:, :SA] = pair.sig_ab, pair.sig_ab.T
        self._u0 = {}

    def x_terms(self, mol_a, mol_b, box):
        """(x_lj, x_real, x_recip, overlap) of A [S_A + 1][3] and B [S_B + 1][3] alone in the box."""
        orc, p = self.orc, self.pair
        SA, SB, L = p.a.n_sites, p.b.n_sites, float(box)
        mol_a, mol_b = np.asarray(mol_a, dtype=float).reshape(SA + 1, 3), np.asarray(mol_b, dtype=float).reshape(SB + 1, 3)
        q = np.concatenate([p.a.charge, p.b.charge])
        coords = np.vstack([mol_a[:SA], mol_b[:SB]])
        s = orc.System(np.vstack([mol_a[SA], mol_b[SB]]), np.array([1, SA + 1], dtype=np.int64),
                       np.array([SA, SA + SB], dtype=np.int64), coords, np.arange(1, SA + SB + 1, dtype=np.int64), q,
                       self.eps, self.sig, L)
        ew = orc.Ewald(self.alpha / L, 5, 27, L, factor=structs.factor)
        lj, _ = orc.lj_poly_du(2, s, self.lj_rcut)
        real, _, ov = orc.ewald_short(2, s, ew, self.qq_rcut)
        rl = orc.recip_long(ew, coords, q, L)
        rl -= orc.recip_long(ew, coords[:SA], q[:SA], L)
        rl -= orc.recip_long(ew, coords[SA:], q[SA:], L)
        return lj, real, ew.factor * rl, ov

    def total_difference(self, com, coords, mol_a, mol_b, box, key=None):
        """The oracle's potential(N + 2) - potential(N) with A and B appended, and the larger magnitude
        of the two totals.  `key`: a name under which potential(N) of this configuration is kept."""
        orc, p = self.orc, self.pair
        SA, SB, n, L = p.a.n_sites, p.b.n_sites, com.shape[0], float(box)
        mol_a, mol_b = np.asarray(mol_a, dtype=float).reshape(SA + 1, 3), np.asarray(mol_b, dtype=float).reshape(SB + 1, 3)
        nt = 3 + SA + SB
        eps, sig = np.zeros((nt, nt)), np.zeros((nt, nt))
        eps[:3 + SA, :3 + SA], sig[:3 + SA, :3 + SA] = self.oa.eps, self.oa.sig
        eps[3 + SA:, :3], eps[:3, 3 + SA:] = p.b.eps, p.b.eps.T
        sig[3 + SA:, :3], sig[:3, 3 + SA:] = p.b.sig, p.b.sig.T
        eps[3:3 + SA, 3 + SA:], eps[3 + SA:, 3:3 + SA] = p.eps_ab, p.eps_ab.T
        sig[3:3 + SA, 3 + SA:], sig[3 + SA:, 3:3 + SA] = p.sig_ab, p.sig_ab.T
        w = 3 * np.arange(n, dtype=np.int64)
        q0 = np.asarray(self.a["charge"][:3 * n], dtype=float)
        at0 = np.tile([1, 2, 3], n).astype(np.int64)
        ew = orc.Ewald(self.alpha / L, 5, 27, L, factor=structs.factor)
        s0 = orc.System(com, w + 1, w + 3, coords, at0, q0, eps, sig, L)
        s2 = orc.System(np.vstack([com, mol_a[SA], mol_b[SB]]), np.concatenate([w + 1, [3 * n + 1, 3 * n + SA + 1]]),
                        np.concatenate([w + 3, [3 * n + SA, 3 * n + SA + SB]]), np.vstack([coords, mol_a[:SA], mol_b[:SB]]),
                        np.concatenate([at0, 4 + np.arange(SA + SB)]).astype(np.int64),
                        np.concatenate([q0, p.a.charge, p.b.charge]), eps, sig, L)
        u2 = orc.potential_ewald(s2, ew, self.lj_rcut, self.qq_rcut)["energy"]
        if key is None or key not in self._u0:
            self._u0[key] = orc.potential_ewald(s0, ew, self.lj_rcut, self.qq_rcut)["energy"]
        u0 = self._u0[key]
        return u2 - u0, max(abs(u2), abs(u0))

    def reference(self, com, coords, mol_a, mol_b, box, key=None):
        """Rows [1 + 2 K][3] and flags [1 + K] (bits 0 and 2) of one insertion: A [S_A + 1][3] and B
        [K][S_B + 1][3]."""
        K = mol_b.shape[0]
        rows, flags = np.zeros((1 + 2 * K, 3)), np.zeros(1 + K, dtype=np.uint8)
        *rows[0], ov = self.oa.terms(com, coords, mol_a, box, key=key)
        flags[0] = 1 if ov else 0
        for k in range(K):
            *rows[1 + k], ov = self.ob.terms(com, coords, mol_b[k], box, key=key)
            *rows[1 + K + k], ovx = self.x_terms(mol_a, mol_b[k], box)
            flags[1 + k] = (1 if ov else 0) | (4 if ovx else 0)
        return rows, flags


def expected_flags(rows, ofl):
    """The flag bytes [1 + K] k_pair_reduce leaves for an insertion whose rows [1 + 2 K][3] and
    overlap bits ofl [1 + K] (0 and 2) are the oracle's: bit 1 where dU_A (column 0) or dU_B is
    non-finite, bit 3 where dU_AB = (dU_A + dU_B) + x is."""
    K = ofl.shape[0] - 1
    with np.errstate(invalid="ignore"):
        du_a, du_b, _, du_ab = du_total(rows)
    out = np.zeros(1 + K, dtype=np.uint8)
    out[0] = (int(ofl[0]) & 1) | (0 if np.isfinite(du_a) else 2)
    for k in range(K):
        out[1 + k] = (int(ofl[1 + k]) & 5) | (0 if np.isfinite(du_b[k]) else 2) | (0 if np.isfinite(du_ab[k]) else 8)
    return out


def check_pair(po, b, r, mol_a, mol_b, du, flags, what="", cache=True, nonfinite=None):
    """Every term and the overlap bits of replica r's insertions against the oracle, on the replica's
    own coordinates: solute_ref.solute_close with S = S_A for A, S_B for B and S_A + S_B for x.
    Returns the oracle's rows [M][1 + 2 K][3] and flags [M][1 + K].
    cache=False: recip_long(N) is recomputed for every placement (after anything that changed the
    committed state a kept value would hide what is sought).  `nonfinite`: a list; a row (j, row)
    whose oracle terms are not all finite (a site planted exactly on another) is appended to it, its
    terms are not compared and the library's dU of the row must be non-finite; and EVERY flag byte
    must then be expected_flags of the oracle's rows, all four bits."""
    com, coords, _ = b.get_replica(r)
    box = float(b.get_boxes()[r])
    SA, SB = po.pair.a.n_sites, po.pair.b.n_sites
    Mi, K = mol_b.shape[0], mol_b.shape[1]
    bad, ref, rfl = [], [], []
    for j in range(Mi):
        rows, fl = po.reference(com, coords, mol_a[j], mol_b[j], box, key=(id(b), r) if cache else None)
        ref.append(rows)
        rfl.append(fl)
        for e in range(1 + K):
            if (int(flags[j, e]) & 5) != int(fl[e]):
                bad.append((j, e, "flags", int(flags[j, e]), int(fl[e])))
        if nonfinite is not None:
            want = expected_flags(rows, fl)
            if not np.array_equal(flags[j], want):
                bad.append((j, "flag bytes", flags[j].tolist(), want.tolist()))
        for row in range(1 + 2 * K):
            S = SA if row == 0 else SB if row <= K else SA + SB
            if nonfinite is not None and not np.all(np.isfinite(rows[row])):
                nonfinite.append((j, row))
                if np.isfinite((du[j, row, 0] + du[j, row, 1]) + du[j, row, 2]):
                    bad.append((j, row, "finite dU", tuple(du[j, row])))
                continue
            for c, name in enumerate(("lj", "real", "recip")):
                if not sr.solute_close(du[j, row, c], rows[row, c], S):
                    bad.append((j, row, name, du[j, row, c], rows[row, c]))
    assert not bad, f"{what} {po.pair} replica {r}: {bad[:6]}"
    return np.array(ref), np.array(rfl)


def du_total(rows):
    """dU_A [..], dU_B [.., K], x [.., K] and dU_AB [.., K] from rows [.., 1 + 2 K, 3], in the
    library's order of additions."""
    K = (rows.shape[-2] - 1) // 2
    t = (rows[..., 0] + rows[..., 1]) + rows[..., 2]
    du_a, du_b, x = t[..., 0], t[..., 1:1 + K], t[..., 1 + K:]
    return du_a, du_b, x, (du_a[..., None] + du_b) + x


def host_sums(du, flags, sums0, temperature):
    """The in-order reductions the library promises (common.widom_host_sums per column), from du
    (R, M, 1 + 2 K, 3) and the flags the library returned (R, M, 1 + K), added to copies of sums0."""
    K = flags.shape[2] - 1
    out = {k: np.array(v).copy() for k, v in sums0.items()}
    out["boltz_a"], out["n_zero_a"] = common.widom_host_sums(du[:, :, 0], flags[:, :, 0], sums0["boltz_a"],
                                                             sums0["n_zero_a"], temperature)
    du_a, du_b, x, _ = du_total(du)
    for k in range(K):
        out["boltz_b"][:, k], out["n_zero_b"][:, k] = common.widom_host_sums(
            du[:, :, 1 + k], flags[:, :, 1 + k] & 3, sums0["boltz_b"][:, k], sums0["n_zero_b"][:, k], temperature)
        three = np.stack([du_a, du_b[:, :, k], x[:, :, k]], axis=2)
        out["boltz_ab"][:, k], out["n_zero_ab"][:, k] = common.widom_host_sums(
            three, flags[:, :, 0] | flags[:, :, 1 + k], sums0["boltz_ab"][:, k], sums0["n_zero_ab"][:, k], temperature)
    return out


# ---- inputs shared by test_solute_pair_host.py (preconditions) and test_gpu_solute_pair.py ----------
def edge_pair(a):
    return synthetic_pair(a, 3, 4)


def edge_cases(a, pair, com, coords):
    """Placements for mmc_batch_widom_pair_at in the starting configuration (com, coords) of system
    `a`, K = 2 each: (mol_a (1, n, S_A + 1, 3), mol_b (1, n, 2, S_B + 1, 3), names).  Sites straddling
    faces; c_A at 0 and at L; c_B on either side of A's gate (RCUT) by factors 1 -+ 1e-12; a site of B
    on a water hydrogen of the opposite charge (the last case, placement 0)."""
    L = float(a["box"])
    oa, ob = pair.a.offsets, pair.b.offsets

    def up(off, c):
        c = np.asarray(c, dtype=float)
        return np.vstack([c + off, c])

    u = np.array([2.0, -1.0, 2.0]) / 3.0
    v = np.array([0.6, 0.0, 0.8])
    cases = []
    for name, ca in (("faces", [0.2, L - 0.3, 15.0]), ("corner", [L - 0.1, 0.05, L - 0.2]), ("zero", [0.0, 0.0, 0.0]),
                     ("box", [L, L, L]), ("mixed", [L, 7.0, 0.0])):
        ca = np.asarray(ca)
        cases.append((name, up(oa, ca), [up(ob, (ca + 3.3 * u) % L), up(ob, (ca - 6.1 * v) % L)]))
    for j in (3, 411):
        ca = com[j] + np.array([0.3, -0.2, 0.1])
        for f in (1 - 1e-12, 1 + 1e-12):
            cases.append((f"gate{j}", up(oa, ca % L), [up(ob, (ca + RCUT * f * u) % L), up(ob, (ca - RCUT * f * v) % L)]))
    neg = int(np.argmin(pair.b.charge))
    assert pair.b.charge[neg] < 0 < a["charge"][1]
    cb = coords[3 * 100 + 1] - ob[neg]
    cases.append(("overlap", up(oa, (cb + 4.0 * u) % L), [up(ob, cb), up(ob, (cb + 5.0 * v) % L)]))
    mol_a = np.array([c[1] for c in cases])[None]
    mol_b = np.array([c[2] for c in cases])[None]
    return mol_a, mol_b, [c[0] for c in cases]


FLUSH_RCUT = 12.4


def dense_water(n_mol=2000, rho=0.06, seed=5):
    """The dense system of test_gpu_solute.py's test_neighbour_list_flush: 2000 SPC/E molecules on the
    crystal start compressed to 0.06 / A^3 (32.2 A)."""
    from metropolismontecarlo_amd import io as mio
    box, com, coords = mio.cubic_lattice_water(n_mol, rho, "spce", seed=seed)
    a4 = common.nist_arrays(4, "unwrapped")
    first = 3 * np.arange(n_mol, dtype=np.int64) + 1
    return dict(com=com, coords=coords, first_atom=first, last_atom=first + 2,
                atype=np.tile([1, 2, 2], n_mol).astype(np.int64),
                charge=np.tile([mio.SPCE_Q_O, mio.SPCE_Q_H, mio.SPCE_Q_H], n_mol), eps=a4["eps"],
                sig=a4["sig"], box=float(box))


def flush_cases(a, pair, n=6, d=(3.0, 5.0, 7.0, 9.0, 11.0)):
    """n insertions for _at into the dense system, A at the centres of lattice cells and B at K = 5
    separations along random rays, random orientations: (mol_a (1, n, ..), mol_b (1, n, K, ..))."""
    L = float(a["box"])
    nc = int(round(np.cbrt(2197)))
    sp = L / nc
    rng = np.random.default_rng(2001)
    cells = rng.choice(nc ** 3, size=n, replace=False)

    def rot():
        q = rng.normal(size=4)
        w, x, y, z = q / np.linalg.norm(q)
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                         [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])

    mol_a, mol_b = [], []
    for c in cells:
        i, j, k = c // (nc * nc), (c // nc) % nc, c % nc
        ca = (np.array([i, j, k]) + 0.51) * sp
        mol_a.append(np.vstack([ca + pair.a.offsets @ rot().T, ca]))
        nh = rng.normal(size=3)
        nh /= np.linalg.norm(nh)
        rb = pair.b.offsets @ rot().T
        mol_b.append([np.vstack([(ca + dk * nh) % L + rb, (ca + dk * nh) % L]) for dk in d])
    return np.array(mol_a)[None], np.array(mol_b)[None]


# ---- inputs shared by test_solute_paths_host.py (preconditions) and test_gpu_solute_paths.py --------
SUMS = ("boltz_a", "n_zero_a", "boltz_b", "n_zero_b", "boltz_ab", "n_zero_ab")
PATH_D = (3.0, 5.0, 7.0, 9.0, 11.0)       # two tiles, the last separation beyond both gates (r_cut 10)
SMALL_D = (2.5, 4.0, 5.5, 7.5, 9.2)       # ... in the 18.7 A boxes (r_cut 7 and 9), below half the box
SMALL_N = (1, 2, 63, 64, 65, 256, 257)
GEN_D, GEN_SEED, GEN_DRAW0, GEN_M = (1.0, 7.0, 14.9), 93, 2 ** 32 - 3, 8
FLAG_SEED, FLAG_M, FLAG_D = 4712, 200, (3.0, 6.0, 11.0)


def path_solute(a):
    return sr.synthetic(a, 5, seed=5)


def path_pair(a):
    return synthetic_pair(a, 3, 4)


def flag_pair(a):
    """The pair of the planted flags: both solutes have a negative site with LJ (a site on a water
    oxygen then overlaps nothing) and site pairs of either sign of q_a q_b with eps_ab > 0."""
    return synthetic_pair(a, 5, 4)


def full_pair(a, SA=8, SB=8):
    """synthetic(SA) with synthetic(SB) and a cross table without a zeroed entry."""
    A, B = sr.synthetic(a, SA, seed=SA), sr.synthetic(a, SB, seed=SB)
    rng = np.random.default_rng(100 * SA + SB)
    return structs.SolutePair(A, B, 30.0 + 70.0 * rng.random((SA, SB)), 2.5 + rng.random((SA, SB)))


def mixed_pair(a, methane_first):
    """United-atom methane with solute_ref.dipole: exactly one solute of the pair is charged."""
    p = structs.SolutePair(sr.methane(a), sr.dipole(a), *cross([147.9], [3.73], [110.0, 0.0], [3.4, 0.0]))
    return p if methane_first else p.swapped()


def separations(K):
    return (4.0,) if K == 1 else tuple(np.linspace(2.5, 14.9, K))


def pair_gate_cases(mol_a, box, pair, lj, qq, seed=17):
    """For each given A [n][S_A + 1][3] K = 4 placements of B, c_B at (1 - 1e-12) g, (1 + 1e-12) g of
    the smaller gate and then of the larger, from c_A along solute_ref.GATE_DIRS[i % 3], one random
    orientation per insertion: separation 0 is inside both gates, 1 and 2 between them, 3 outside."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(mol_a.shape[0]):
        rot, u = sr.rotation(rng), sr.GATE_DIRS[i % 3]
        out.append([sr.placed(pair.b.offsets, (mol_a[i, -1] + g * f * u) % box, rot)
                    for g in sorted((lj, qq)) for f in (1 - 1e-12, 1 + 1e-12)])
    return np.array(out)


def gate_pattern(x, lj, qq):
    """Whether x [n][4][3], the x rows of pair_gate_cases, switch as the gates say: inside both gates
    x_lj and x_real are non-zero, outside both they are zero, between them only the term of the
    larger gate is non-zero."""
    x_lj, x_real = x[:, :, 0] != 0.0, x[:, :, 1] != 0.0
    between_lj, between_real = (lj > qq), (qq > lj)
    return bool(np.all(x_lj[:, 0]) and np.all(x_real[:, 0]) and not x_lj[:, 3].any() and not x_real[:, 3].any()
                and np.all(x_lj[:, 1:3] == between_lj) and np.all(x_real[:, 1:3] == between_real))


def small_cases(a, n, sol, pair, d=PATH_D):
    """_at placements in the first n molecules of system `a`: the reference point 3 A from molecule
    n - 1's COM (the index the scans' clamp protects), B along another direction: (mol (1, 1, S + 1,
    3), mol_a (1, 1, S_A + 1, 3), mol_b (1, 1, K, S_B + 1, 3))."""
    L = float(a["box"])
    c = (np.asarray(a["com"])[n - 1] + 3.0 * np.array([2.0, -1.0, 2.0]) / 3.0) % L
    v = np.array([0.6, 0.0, 0.8])
    mol_b = np.array([sr.placed(pair.b.offsets, (c + dk * v) % L) for dk in d])
    return sr.placed(sol.offsets, c)[None, None], sr.placed(pair.a.offsets, c)[None, None], mol_b[None, None]


def overlaps_ab(sites_a, q_a, sites_b, q_b, box, ovr=0.5):
    d = np.asarray(sites_a, dtype=float)[:, None, :] - np.asarray(sites_b, dtype=float)[None, :, :]
    d = d + common.image_shift(d, box)
    return bool(np.any(((d * d).sum(2) < ovr) & (np.asarray(q_a)[:, None] * np.asarray(q_b)[None, :] < 0)))


HOT_T, HOT_SEED, HOT_M, HOT_D = 5000.0, 4713, 65, (3.0, 6.0)


def hot_pair(a):
    """solute_ref.dipole (its negative site has no LJ) with a ghost: dU_AB is dU_A."""
    return structs.SolutePair(sr.dipole(a), ghost(2), np.zeros((2, 2)), np.zeros((2, 2)))


def light_overlap(a, sol, coords, seed=29):
    """`sol` [S + 1][3] with its negative LJ-free site 0.5 A from a water H, no other site within
    sqrt(0.5) A of an opposite charge and every LJ site at least 2.4 A from every oxygen: an overlap
    (flag bit 0, d_real = 0) whose dU = d_lj + d_recip stays moderate, so that at HOT_T the weight it
    would have WITHOUT its flag is of the order of the other insertions' weights."""
    L = float(a["box"])
    rng = np.random.default_rng(seed)
    q_w = np.asarray(a["charge"], dtype=float)[:coords.shape[0]]
    neg = int(np.argmin(sol.charge))
    assert sol.charge[neg] < 0 < q_w[1] and sol.eps[neg].max() <= 0.001
    lj = sol.eps[:, 0] > 0.001
    rest = np.arange(sol.n_sites) != neg
    oxy = coords[0::3]
    arm = sol.offsets[lj].mean(0) - sol.offsets[neg]        # from the negative site to the LJ sites
    arm = arm / np.linalg.norm(arm)
    for w in rng.permutation(coords.shape[0] // 3)[:200]:
        for h in (1, 2):
            out = coords[3 * w + h] - coords[3 * w]
            out = out + common.image_shift(out, L)
            out = out / np.linalg.norm(out)                 # O -> H: the way out of this water
            for _ in range(50):
                rot, v = sr.rotation(rng), out + 0.4 * rng.normal(size=3)
                if (rot @ arm) @ out < 0.8:
                    continue
                target = coords[3 * w + h] + 0.5 * v / np.linalg.norm(v)
                m = sr.placed(sol.offsets, target - sol.offsets[neg] @ rot.T, rot)
                m[neg] = target
                d = m[:-1][lj][:, None, :] - oxy[None, :, :]
                d = d + common.image_shift(d, L)
                if (d * d).sum(2).min() >= 2.4 ** 2 and not sr.overlaps_water(m[:-1][rest], sol.charge[rest], coords, q_w, L):
                    return m
    raise AssertionError("no placement found")


def flag_plants(a, pair, coords, mol_a, mol_b, r=0, seed=23):
    """Plants the flagged placements of the test of k_pair_reduce's later blocks into mol_a [M][S_A + 1][3]
    and mol_b [M][K][S_B + 1][3] (M >= 192, K = 3) of one replica with atoms `coords`, in place.
    Returns {(j, column): flag byte}; the kinds, each oriented at random until no OTHER flag of the
    planted placement can arise (no further site within sqrt(0.5) A of an opposite charge):
      A  a negative site 0.5 A from a water H                    (j = 5, 70)   column 0: bit 0
      A  a negative LJ site exactly on a water O                 (j = 100)     column 0: bit 1; every
                                                                               column 1 + k: bit 3 on top
      B_1 a negative site 0.5 A from a water H                   (j = 128)     column 2: bit 0
      B_2 a negative LJ site exactly on a water O                (j = 140)     column 3: bits 1 and 3
      B_0 a site 0.5 A from an A site of the opposite charge     (j = 191)     column 1: bit 2 only
      B_2 a site exactly on an A site, eps_ab > 0, q_a q_b >= 0  (j = 150)     column 3: bit 3 only
    For the last two, A is the insertion's own (generated) one, and j moves down from the stated one
    until B fits among the waters."""
    L = float(a["box"])
    rng = np.random.default_rng(seed + r)
    q_w = np.asarray(a["charge"], dtype=float)[:coords.shape[0]]
    A, B = pair.a, pair.b
    SA, SB = A.n_sites, B.n_sites

    def lj_negative(s):
        i = [k for k in range(s.n_sites) if s.charge[k] < 0 and s.eps[k, 0] > 0.001]
        assert i, s
        return i[0]

    def unit():
        v = rng.normal(size=3)
        return v / np.linalg.norm(v)

    def at_water(s, site, target, others_free):
        """s with its `site` on `target`, no other opposite-charge contact with the waters."""
        for _ in range(400):
            rot = sr.rotation(rng)
            m = sr.placed(s.offsets, target - s.offsets[site] @ rot.T, rot)
            m[site] = target
            keep = np.arange(s.n_sites) != site if others_free else np.ones(s.n_sites, dtype=bool)
            if not sr.overlaps_water(m[:-1][keep], s.charge[keep], coords, q_w, L):
                return m
        raise AssertionError("no orientation found")

    plant = {}
    neg_a, neg_b = int(np.argmin(A.charge)), int(np.argmin(B.charge))
    assert A.charge[neg_a] < 0 and B.charge[neg_b] < 0 < q_w[1]
    for j, w in ((5, 100), (70, 101)):
        mol_a[j] = at_water(A, neg_a, coords[3 * (w + r) + 1] + 0.5 * unit(), True)
        plant[(j, 0)] = 1
    mol_a[100] = at_water(A, lj_negative(A), coords[3 * (200 + r)].copy(), False)
    plant[(100, 0)] = 2
    mol_b[128, 1] = at_water(B, neg_b, coords[3 * (300 + r) + 1] + 0.5 * unit(), True)
    plant[(128, 2)] = 1
    mol_b[140, 2] = at_water(B, lj_negative(B), coords[3 * (400 + r)].copy(), False)
    plant[(140, 3)] = 2 | 8
    # the A-B plants
    qq = A.charge[:, None] * B.charge[None, :]
    ia, ib = np.argwhere(qq < 0)[0]
    ja, jb = np.argwhere((qq >= 0) & (pair.eps_ab > 0.001))[0]
    for j0, k, sa, sb, gap, byte in ((191, 0, ia, ib, 0.5, 4), (150, 2, ja, jb, 0.0, 8)):
        done = False
        for j in range(j0, j0 - 20, -1):
            ma = mol_a[j]
            if sr.overlaps_water(ma[:-1], A.charge, coords, q_w, L):
                continue                  # (an A that overlaps a water weighs 0 anyway: take a plain one)
            for _ in range(200):
                rot = sr.rotation(rng)
                target = ma[sa] + gap * unit()
                m = sr.placed(B.offsets, target - B.offsets[sb] @ rot.T, rot)
                m[sb] = target
                rest = np.arange(SB) != sb
                far = np.linalg.norm(m[:-1][rest][None] - ma[:-1][:, None], axis=2).min() > 0.05
                if (not sr.overlaps_water(m[:-1], B.charge, coords, q_w, L) and far
                        and np.linalg.norm(m[:-1][:, None] - coords[None], axis=2).min() > 0.8
                        and overlaps_ab(ma[:-1], A.charge, m[:-1], B.charge, L) == (byte == 4)):
                    mol_b[j, k] = m
                    plant[(j, 1 + k)] = byte
                    done = True
                    break
            if done:
                break
        assert done, (j0, k)
    return plant
