"""Helpers of the solute-pair tests (test_solute_pair_abi.py, test_solute_pair_host.py,
test_gpu_solute_pair.py): the pairs the tests insert and the oracle's statement of every term --
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


def check_pair(po, b, r, mol_a, mol_b, du, flags, what=""):
    """Every term and the overlap bits of replica r's insertions against the oracle, on the replica's
    own coordinates: solute_ref.solute_close with S = S_A for A, S_B for B and S_A + S_B for x.
    Returns the oracle's rows [M][1 + 2 K][3] and flags [M][1 + K]."""
    com, coords, _ = b.get_replica(r)
    box = float(b.get_boxes()[r])
    SA, SB = po.pair.a.n_sites, po.pair.b.n_sites
    Mi, K = mol_b.shape[0], mol_b.shape[1]
    bad, ref, rfl = [], [], []
    for j in range(Mi):
        rows, fl = po.reference(com, coords, mol_a[j], mol_b[j], box, key=(id(b), r))
        ref.append(rows)
        rfl.append(fl)
        for e in range(1 + K):
            if (int(flags[j, e]) & 5) != int(fl[e]):
                bad.append((j, e, "flags", int(flags[j, e]), int(fl[e])))
        for row in range(1 + 2 * K):
            S = SA if row == 0 else SB if row <= K else SA + SB
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
