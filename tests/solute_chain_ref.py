"""Helpers of the fixed-solute tests (test_solute_chain_abi.py, test_solute_chain_host.py,
test_gpu_solute_chain.py, test_gpu_solute_chain_paths.py): the numpy restatement of
mmc_batch_rdf_solute, the FNV-1a fingerprint of a solute (mmc_state_info::solute_hash), and the
oracle's N + 1 molecule system -- the batch's waters with the solute appended as molecule N + 1 with
its own atom types, as solute_ref.SoluteOracle appends it -- with the trial moves, totals and chains of
that system."""
import math

import numpy as np

from metropolismontecarlo_amd import structs

T = 298.15


# ---- mmc_batch_rdf_solute ---------------------------------------------------------------------------
def rdf_solute_ref(mol, coords, box, numbins, r_max=0.0):
    """Counts [1 + S][3][numbins] of one frame: row 0 from the reference point mol[S], row 1 + a from
    site a, against the three water slots, in mmc_batch_rdf_sites' arithmetic (gr.jl:75-90): d = point
    - site, |d| > box / 2 (strict) moves d by one box, r = sqrt((xx xx + yy yy) + zz zz), bin =
    ceil(r / dr), counted at [bin - 1] when 1 <= bin <= numbins; dr = r_max / numbins, or (box / 2) /
    numbins for r_max <= 0."""
    mol = np.asarray(mol, dtype=float)
    S = mol.shape[0] - 1
    dr = r_max / numbins if r_max > 0.0 else (box / 2.0) / numbins
    pts = np.vstack([mol[S:], mol[:S]])
    w = np.asarray(coords, dtype=float).reshape(-1, 3, 3)
    d = pts[:, None, None, :] - w[None, :, :, :]
    d = np.where(d > box / 2.0, d - box, np.where(d < -box / 2.0, d + box, d))
    r = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    b = np.ceil(r / dr).astype(np.int64)                       # [1 + S][N][3]
    hist = np.zeros((1 + S, 3, numbins), dtype=np.uint64)
    for row in range(1 + S):
        for slot in range(3):
            bb = b[row, :, slot]
            bb = bb[(bb >= 1) & (bb <= numbins)]
            hist[row, slot] = np.bincount(bb - 1, minlength=numbins).astype(np.uint64)
    return hist


# ---- mmc_state_info::solute_hash --------------------------------------------------------------------
def solute_hash(solute, mol):
    """FNV-1a (64 bit) over n_sites (8 bytes, little endian) and the bytes of mol [S + 1][3], charge
    [S], eps [S][3], sig [S][3]."""
    S = solute.n_sites
    raw = np.int64(S).tobytes()
    for arr, shape in ((mol, (S + 1, 3)), (solute.charge, (S,)), (solute.eps, (S, 3)), (solute.sig, (S, 3))):
        raw += np.ascontiguousarray(arr, dtype=np.float64).reshape(shape).tobytes()
    h = 0xcbf29ce484222325
    for c in raw:
        h = ((h ^ c) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


# ---- the oracle's N + 1 system ----------------------------------------------------------------------
class N1:
    """The waters (com, coords) of system `a` with the solute `so.sol` (a solute_ref.SoluteOracle: its
    tables, cutoffs and alpha) placed at mol [S + 1][3] as molecule N + 1: an oracle.System, its Ewald
    with S(k) of all N + 1 molecules, and the calls the tests make on it."""

    def __init__(self, so, com, coords, mol, box):
        orc, sol = so.orc, so.sol
        self.so, self.orc = so, orc
        S, n, L = sol.n_sites, np.asarray(com).shape[0], float(box)
        self.S, self.n, self.box = S, n, L
        mol = np.asarray(mol, dtype=float).reshape(S + 1, 3)
        first = np.concatenate([3 * np.arange(n, dtype=np.int64) + 1, [3 * n + 1]])
        last = np.concatenate([3 * np.arange(n, dtype=np.int64) + 3, [3 * n + S]])
        atype = np.concatenate([np.tile([1, 2, 3], n), 4 + np.arange(S)]).astype(np.int64)
        q = np.concatenate([np.asarray(so.a["charge"][:3 * n], dtype=float), sol.charge])
        self.s = orc.System(np.vstack([np.asarray(com, dtype=float).reshape(n, 3), mol[S]]), first, last,
                            np.vstack([np.asarray(coords, dtype=float).reshape(3 * n, 3), mol[:S]]), atype, q,
                            so.eps, so.sig, L)
        self.ew = orc.Ewald(so.alpha / L, 5, 27, L, factor=structs.factor)
        self.recip_long()

    def recip_long(self):
        return self.orc.recip_long(self.ew, self.s.coords, self.s.charge, self.box)

    def potential(self):
        return self.orc.potential_ewald(self.s, self.ew, self.so.lj_rcut, self.so.qq_rcut)

    def trial(self, i, com_new, atoms_new):
        """((d_lj, d_real, d_recip, d_vir), overlap) of moving water i (1-based); S(k) new is left in
        the Ewald's sumQExpNew (commit() or rollback() follows)."""
        return self.orc.trial_move(i, self.s, self.ew, self.so.lj_rcut, self.so.qq_rcut, com_new, atoms_new)

    def commit(self, i, com_new, atoms_new):
        self.s.com[i - 1] = com_new
        self.s.coords[3 * i - 3:3 * i] = atoms_new
        self.ew.sumQExpOld = self.ew.sumQExpNew.copy()

    def rollback(self):
        self.ew.sumQExpNew = self.ew.sumQExpOld.copy()

    def pair_energy(self):
        """(u_lj, u_real, overlap) of the solute against all waters: LJ_poly_dU(N + 1), EwaldShort(N + 1)."""
        lj, _ = self.orc.lj_poly_du(self.n + 1, self.s, self.so.lj_rcut)
        real, _, ov = self.orc.ewald_short(self.n + 1, self.s, self.ew, self.so.qq_rcut)
        return lj, real, bool(ov)


# ---- the driver's own draws (host proposals) --------------------------------------------------------
M64 = 0xFFFFFFFFFFFFFFFF


class HostRng:
    """The native driver's generator of one replica (mmc_engine.inc, struct Rng and run_prepare):
    xoshiro256++ seeded by splitmix64 from a hash of (seed, global replica index, steps the batch
    had run before the call); uniform() = (next() >> 11) 2^-53."""

    def __init__(self, seed, replica, steps_done=0):
        self.x = seed & M64
        h = self._splitmix() ^ (replica & M64)
        self.x = h
        h = self._splitmix() ^ (steps_done & M64)
        self.x = h
        self.s = [self._splitmix() for _ in range(4)]

    def _splitmix(self):
        self.x = (self.x + 0x9e3779b97f4a7c15) & M64
        z = self.x
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
        return z ^ (z >> 31)

    @staticmethod
    def _rotl(x, k):
        return ((x << k) | (x >> (64 - k))) & M64

    def next(self):
        s = self.s
        result = (self._rotl((s[0] + s[3]) & M64, 23) + s[0]) & M64
        t = (s[1] << 17) & M64
        s[2] ^= s[0]
        s[3] ^= s[1]
        s[1] ^= s[2]
        s[0] ^= s[3]
        s[2] ^= t
        s[3] = self._rotl(s[3], 45)
        return result

    def uniform(self):
        return float(self.next() >> 11) * 2.0 ** -53


def host_proposal(rng, box, dr_max, dphi_max):
    """proposal(step, com, atoms) of replay() for a chain whose moves the driver proposes on the host
    (mmc_engine.inc, propose(): random_translate_vector of auxillary.jl:94-103 with boundaries.jl's
    wrap, or a rotation about a random axis found by rejection, quaternions.jl:52-74, by an angle
    uniform in +-dphi_max), in its arithmetic and its order of draws.  The Metropolis uniform is the
    NEXT draw of the same generator, taken only when dU / T >= 0 (Driver::decide): returned as a
    callable."""
    def pbc1(x):
        if x > box:
            x -= box
        if x < 0:
            x += box
        return x

    def proposal(step, com, atoms):
        if rng.uniform() < 0.5:
            c_new = np.array([pbc1(com[k] + (rng.uniform() - 0.5) * dr_max) for k in range(3)])
            return 0, c_new, atoms + (c_new - com), rng.uniform
        while True:
            e = np.array([2.0 * rng.uniform() - 1.0 for _ in range(3)])
            norm = e[0] * e[0] + e[1] * e[1] + e[2] * e[2]
            if norm < 1.0 and norm != 0.0:
                break
        e = e * (1.0 / math.sqrt(norm))
        angle = (2.0 * rng.uniform() - 1.0) * dphi_max
        c, s = math.cos(angle), math.sin(angle)
        t = 1.0 - c
        Rm = [[t * e[0] * e[0] + c, t * e[0] * e[1] - s * e[2], t * e[0] * e[2] + s * e[1]],
              [t * e[0] * e[1] + s * e[2], t * e[1] * e[1] + c, t * e[1] * e[2] - s * e[0]],
              [t * e[0] * e[2] - s * e[1], t * e[1] * e[2] + s * e[0], t * e[2] * e[2] + c]]
        a_new = np.empty((3, 3))
        for a in range(3):
            o = atoms[a] - com
            for k in range(3):
                a_new[a, k] = com[k] + Rm[k][0] * o[0] + Rm[k][1] * o[1] + Rm[k][2] * o[2]
        return 1, com.copy(), a_new, rng.uniform
    return proposal


def replay(n1, proposal, n_steps, temperature, step0=0):
    """The chain of the N + 1 system through n_steps steps: step k moves water k % N with
    proposal(step0 + k, com, atoms) -> (kind, com_new, atoms_new, u), u the Metropolis uniform or a
    callable that draws it (called only when dU / T >= 0); Metropolis as main.jl:593-598.
    Returns the trace [(dU, flags)] (bit 0 accepted, bit 1 overlap, bit 2 rotation), the sum of the
    accepted dU and of the accepted virial changes."""
    trace, e_acc, v_acc = [], 0.0, 0.0
    for k in range(n_steps):
        i = k % n1.n
        kind, c_new, a_new, u = proposal(step0 + k, n1.s.com[i].copy(), n1.s.coords[3 * i:3 * i + 3].copy())
        d, ov = n1.trial(i + 1, c_new, a_new)
        delta = d[0] + d[1] + d[2]
        x = delta / temperature
        accept = (x < 0.0 or math.exp(-x) > (u() if callable(u) else u)) and not ov
        trace.append((delta, int(accept) | (int(bool(ov)) << 1) | (kind << 2)))
        if accept:
            e_acc += delta
            v_acc += d[3]
            n1.commit(i + 1, c_new, a_new)
        else:
            n1.rollback()
    return trace, e_acc, v_acc
