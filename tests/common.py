"""Shared helpers for the tests: load the committed fixtures and build matching inputs for the
oracle (oracle.oracle.System / Ewald) and for the product (numpy arrays for device.Context)."""
import json
import os
import re

import numpy as np

from boundary import header_define  # noqa: F401  (tests import it from here)
from metropolismontecarlo_amd import io as mio

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

# NIST SPC/E reference calculations for the four sample configurations (10 A cutoff,
# alpha = 5.6/L, kmax = 5, k^2 < 27); energies / k_B in K.  BASELINE.md section 2.
NIST = {
    1: dict(n=100, L=20.0, disp=9.95387e4, lrc=-8.23715e2, real=-5.58889e5, fourier=6.27009e3,
            self=-2.84469e6, intra=2.80999e6),
    2: dict(n=200, L=20.0, disp=1.93712e5, real=-1.19295e6, fourier=6.03495e3, self=-5.68938e6,
            intra=5.61998e6),
    3: dict(n=300, L=20.0, disp=3.54344e5, real=-1.96297e6, fourier=5.24461e3, self=-8.53407e6,
            intra=8.42998e6),
    4: dict(n=750, L=30.0, disp=4.48593e5, real=-3.57226e6, fourier=7.58785e3, self=-1.42235e7,
            intra=1.41483e7),
}

_golden = None


def nist_arrays(k, variant="reference"):
    return mio.load_nist_fixture(k, variant)


def golden(k, variant="reference"):
    global _golden
    if _golden is None:
        with open(os.path.join(GOLDEN, "golden_oracle.json")) as fh:
            _golden = json.load(fh)
    return _golden[f"config{k}_{variant}"]


def oracle_system(a):
    from oracle import oracle as orc
    return orc.System(a["com"], a["first_atom"], a["last_atom"], a["coords"], a["atype"],
                      a["charge"], a["eps"], a["sig"], a["box"])


def device_context(a, ewald=True):
    from metropolismontecarlo_amd import structs
    from metropolismontecarlo_amd.device import Context
    ctx = Context()
    ctx.upload_system(a["com"], a["first_atom"], a["last_atom"], a["coords"], a["atype"],
                      a["charge"], a["eps"], a["sig"], a["box"])
    if ewald:
        ctx.prepare_ewald(5.6 / a["box"], 5, 27, a["box"], structs.factor)
    return ctx


def rel(a, b, floor=0.0):
    return abs(a - b) / max(abs(b), floor, 1e-300)


def random_system(n_mol, box, seed, na_choices=(3,), n_types=2, min_sep=2.2):
    """A random rigid-molecule system with optionally ragged molecules (na in na_choices), random
    charges (neutral overall), and an LJ table with some zero entries."""
    rng = np.random.default_rng(seed)
    # place COMs on a jittered lattice so that nothing overlaps unless asked for
    nc = int(np.ceil(n_mol ** (1 / 3)))
    d = box / nc
    sites = np.array([(i, j, k) for i in range(nc) for j in range(nc) for k in range(nc)])[:n_mol]
    com = (sites + 0.5) * d + (rng.random((n_mol, 3)) - 0.5) * max(d - min_sep, 0.0) * 0.5
    na = rng.choice(na_choices, size=n_mol)
    first = np.concatenate([[1], 1 + np.cumsum(na)[:-1]]).astype(np.int64)
    last = (first + na - 1).astype(np.int64)
    n_atoms = int(na.sum())
    coords = np.empty((n_atoms, 3))
    for m in range(n_mol):
        off = rng.normal(size=(na[m], 3)) * 0.45
        off -= off.mean(0)
        coords[first[m] - 1:last[m]] = com[m] + off
    atype = rng.integers(1, n_types + 1, size=n_atoms).astype(np.int64)
    charge = rng.normal(size=n_atoms) * 0.5
    charge -= charge.mean()
    e = rng.random(n_types) * 100.0
    e[-1] = 0.0  # a type without LJ, like the SPC/E hydrogens
    s = 2.5 + rng.random(n_types)
    eps = np.sqrt(e[:, None] * e[None, :])
    sig = (s[:, None] + s[None, :]) / 2
    return dict(com=com, first_atom=first, last_atom=last, coords=coords, atype=atype,
                charge=charge, eps=eps, sig=sig, box=float(box))


TIP3P_Q = (-0.834, 0.417, 0.417)   # the SOL charges of tests/golden/decks/topol.top
MIX_ORDERS = ("interleaved", "blocks", "minority1")


def spce_tip3p_mixture(k, order):
    """NIST SPC/E configuration k with some of its molecules made TIP3P waters: a 3-site mixture
    of four atom types (SPC/E O, H = 1, 2; TIP3P O, H = 3, 4), two charge sets and two geometries
    (TIP3P's O-H bonds shortened to 0.9572 A about the oxygen, the centre of mass recomputed with
    the water masses).  `order`: "interleaved" (every other molecule from molecule 2), "blocks"
    (the second half) or "minority1" (molecule 1, the homogeneity template, and every fifth: the
    minority species).  Returns the arrays of the system and the 0/1 species of every molecule."""
    from metropolismontecarlo_amd import structs
    a = mio.load_nist_fixture(k, "unwrapped")
    n = a["com"].shape[0]
    tip = np.zeros(n, dtype=bool)
    if order == "interleaved":
        tip[1::2] = True
    elif order == "blocks":
        tip[n // 2:] = True
    elif order == "minority1":
        tip[::5] = True
    else:
        raise ValueError(order)
    coords = a["coords"].copy().reshape(n, 3, 3)
    com = a["com"].copy()
    m = np.array([15.9994, 1.008, 1.008])
    for j in np.nonzero(tip)[0]:
        o = coords[j, 0]
        coords[j, 1:] = o + (coords[j, 1:] - o) * 0.9572
        com[j] = (coords[j] * m[:, None]).sum(0) / m.sum()
    atype = np.tile([1, 2, 2], n).reshape(n, 3)
    atype[tip] += 2
    charge = np.tile([mio.SPCE_Q_O, mio.SPCE_Q_H, mio.SPCE_Q_H], n).reshape(n, 3)
    charge[tip] = TIP3P_Q
    tab = structs.Tables([mio.SPCE_EPS_O, 0.0, 0.6364 / structs.R, 0.0],
                         [mio.SPCE_SIGMA_O, 0.0, 3.15061, 0.0])
    return dict(a, com=com, coords=coords.reshape(-1, 3), atype=atype.ravel().astype(np.int64),
                charge=charge.ravel(), eps=tab.eps_ij, sig=tab.sig_ij), tip.astype(int)


def mea_tip3p_box(n_water=250, mea_at=(0, 37, 130, 201), rho=0.016, seed=5):
    """The reference's mixture deck (tests/golden/decks: topol.top, mea.pdb, tip3p.pdb): MEA
    molecules (11 atoms) at positions `mea_at` of the molecule list among n_water TIP3P waters, on
    the simple-cubic sites of InitCubicGrid at number density rho with random orientations, and
    the full 13-type table of MakeTables.  Waters follow an MEA in the arrays.  Returns the arrays
    of Context.upload_system (plus "mass")."""
    top = mio.ReadTopFile(os.path.join(GOLDEN, "decks", "topol.top"), substitutions={"SOLNUMBER": 1})
    mea = mio.system_from_decks(mio.ReadPDB(os.path.join(GOLDEN, "decks", "mea.pdb")), top)
    wat = mio.system_from_decks(mio.ReadPDB(os.path.join(GOLDEN, "decks", "tip3p.pdb")), top)
    n_mol = n_water + len(mea_at)
    box, sites = mio.InitCubicGrid(n_mol, rho)
    rng = np.random.default_rng(seed)
    com, coords, atype, charge, mass, first, last = [], [], [], [], [], [], []
    for j in range(n_mol):
        m = mea if j in mea_at else wat
        body = m["coords"] - m["com"][0]
        q = rng.normal(size=4)
        w, x, y, z = q / np.linalg.norm(q)
        rot = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                        [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                        [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        first.append(1 + sum(len(c) for c in coords))
        coords.append(sites[j] + body @ rot.T)
        last.append(first[-1] + len(body) - 1)
        com.append(sites[j])
        atype.append(m["atype"]); charge.append(m["charge"]); mass.append(m["mass"])
    return dict(com=np.array(com, dtype=float), coords=np.concatenate(coords),
                first_atom=np.array(first, dtype=np.int64), last_atom=np.array(last, dtype=np.int64),
                atype=np.concatenate(atype).astype(np.int64), charge=np.concatenate(charge),
                mass=np.concatenate(mass), eps=mea["eps"], sig=mea["sig"], box=float(box))


# ---- which replica k_move_eval_wave runs where ----------------------------------------------------
def _wave_consts():
    """(waves per workgroup, waves per SIMD) of k_move_eval_wave, read from its source so that the
    unit -> wave map below follows the kernel."""
    src = open(os.path.join(HERE, "..", "metropolismontecarlo_amd", "csrc", "mmc_wave.hpp")).read()
    assert re.search(r"#define WV_MWAVES WV_WAVES\b", src)
    return (int(re.search(r"#define WV_WAVES (\d+)", src).group(1)),
            int(re.search(r"#define WV_OCC (\d+)", src).group(1)))


def wave_units(n_units, wave_wgs=0, n_cus=256, occ=None):
    """The units each wave of one k_move_eval_wave launch over n_units takes, in the order it takes
    them: the launch has ceil(n_units / WV_MWAVES) workgroups, capped at option "wave_wgs" or at
    4 * WV_OCC / WV_MWAVES per compute unit (mmc_batch.inc), and wave w of workgroup g loops over
    units g * WV_MWAVES + w, + wgs * WV_MWAVES, ... (mmc_wave.hpp).  Lists in wave order.
    `occ`: the waves per SIMD of the cap when not WV_OCC (k_widom_wave: widom_occ(), whose unit is
    insertion j of replica r, u = r M + j, mmc_widom.inc)."""
    mw, wv_occ = _wave_consts()
    occ = wv_occ if occ is None else occ
    cap = wave_wgs if wave_wgs > 0 else 4 * occ // mw * n_cus
    wgs = min(-(-n_units // mw), cap)
    return [list(range(g * mw + w, n_units, wgs * mw)) for g in range(wgs) for w in range(mw)]


def replicas_by_wave_position(R, n_groups, wave_wgs=0, n_cus=256, parts=1, occ=None):
    """{local replica: where its unit runs} for the replicas worth checking when a wave runs several
    units: in every group (replicas [R g / G, R (g + 1) / G), mmc_engine.inc) the first, second,
    middle and last unit of wave 0 (which runs the most), the last unit of a wave that runs one unit
    fewer, and the group's first and last replica."""
    out = {}
    for g in range(n_groups):
        r0, r1 = R * g // n_groups, R * (g + 1) // n_groups
        waves = wave_units((r1 - r0) * parts, wave_wgs, n_cus, occ)
        w0 = waves[0]
        pos = [(w0[k], 0, k) for k in sorted({0, 1, len(w0) // 2, len(w0) - 1}) if k < len(w0)]
        short = [wv for wv, w in enumerate(waves) if len(w) == len(w0) - 1 and w]
        if short:
            pos.append((waves[short[0]][-1], short[0], len(waves[short[0]]) - 1))
        for u in (0, (r1 - r0) * parts - 1):
            wv = next(k for k, w in enumerate(waves) if u in w)
            pos.append((u, wv, waves[wv].index(u)))
        for u, wv, k in pos:
            out.setdefault(r0 + u // parts, f"group {g}, wave {wv}, unit {k + 1} of {len(waves[wv])}")
    return dict(sorted(out.items()))


def device_cu_count(device=0):
    """Compute units of a device, asked of the HIP runtime the library itself is linked against
    (hipDeviceGetAttribute, looked up through the library's handle)."""
    import ctypes as C
    from metropolismontecarlo_amd import _lib
    get = C.CDLL(_lib.LIB_PATH).hipDeviceGetAttribute
    n = C.c_int(0)
    assert get(C.byref(n), 63, int(device)) == 0   # 63: hipDeviceAttributeMultiprocessorCount
    return n.value


def _wave_list_consts():
    """(WV_LIST, WV_PF) of mmc_wave.hpp: the neighbour-list slots of a wave and the 64-molecule
    blocks of one trip of the COM scan (mmc_wave_unit.inc)."""
    src = open(os.path.join(HERE, "..", "metropolismontecarlo_amd", "csrc", "mmc_wave.hpp")).read()
    return (int(re.search(r"#define WV_LIST (\d+)", src).group(1)),
            int(re.search(r"#define WV_PF (\d+)", src).group(1)))


def widom_occ():
    """WIDOM_OCC of mmc_widom.hpp: the waves per SIMD k_widom_wave's launch is capped at."""
    src = open(os.path.join(HERE, "..", "metropolismontecarlo_amd", "csrc", "mmc_widom.hpp")).read()
    return int(re.search(r"#define WIDOM_OCC (\d+)", src).group(1))


def wolf_occ():
    """WV_OCC_WOLF of mmc_wave.hpp: the waves per SIMD the launch of k_move_eval_wave's Wolf
    instantiations is capped at (mmc_batch.inc)."""
    src = open(os.path.join(HERE, "..", "metropolismontecarlo_amd", "csrc", "mmc_wave.hpp")).read()
    return int(re.search(r"#define WV_OCC_WOLF (\d+)", src).group(1))


def image_shift(d, box):
    """What the minimum image (vector1D, Ewald/boundaries.jl) adds to a coordinate difference d."""
    return np.where(d >= 0.5 * box, -box, np.where(d <= -0.5 * box, box, 0.0))


def scan_flushes(com, centres, gate, box, j_begin=0, j_end=None, exclude=None):
    """Whether the COM scan of mmc_wave_unit.inc certainly empties its neighbour list mid-scan and
    has neighbours left for a later process() call: the unit's centres (one for an insertion, old
    and new COM for a move) scan molecules [j_begin, j_end) in trips of 64 WV_PF; after a trip the
    list is processed and emptied when it holds more than WV_LIST - 64 WV_PF entries.  Counted here
    is the exact gate (a COM within `gate` of a centre, minimum image, by a relative margin of 1e-9
    so that rounding cannot add one) -- a lower bound on the 16-bit prefilter's count.  True when,
    at some trip boundary B, more than that many gated molecules lie before B and at least one
    after it: then some boundary <= B flushes (the count since the last flush cannot stay below
    the threshold), and a later process() call adds to the sums.  `exclude`: a molecule left out
    of both counts (a move's own molecule, which process() drops)."""
    n_list, n_pf = _wave_list_consts()
    com = np.asarray(com, dtype=float)
    j_end = com.shape[0] if j_end is None else j_end
    gated = np.zeros(com.shape[0], dtype=bool)
    for c in np.atleast_2d(centres):
        d = com - np.asarray(c, dtype=float)
        d = d + image_shift(d, box)
        gated |= (d * d).sum(1) < gate * gate * (1 - 1e-9)
    if exclude is not None:
        gated[exclude] = False
    gated[:j_begin] = False
    gated[j_end:] = False
    before = np.cumsum(gated)
    total = int(before[-1]) if before.size else 0
    for b in range(j_begin + 64 * n_pf, j_end, 64 * n_pf):
        if before[b - 1] > n_list - 64 * n_pf and total - before[b - 1] > 0:
            return True
    return False


def image_differs(mol, com, coords, box, gate, slack_sq):
    """Molecules j whose COM is within `gate` of the test molecule mol[12] (atoms, COM) while an
    atom pair of (test, j) takes another minimum image than the molecules' COMs and lies inside
    the slack r^2 < slack_sq in one of the two images: the pairs whose terms the per-molecule image
    of the kernels' IMG variants (mmc_wave_unit.inc; the slack is tested in both) would change."""
    at = np.asarray(mol[:9], dtype=float).reshape(3, 3)
    dc = np.asarray(com) - np.asarray(mol[9:12])
    sc = image_shift(dc, box)
    near = np.nonzero(((dc + sc) ** 2).sum(1) < gate * gate)[0]
    out = []
    for j in near:
        da = coords[3 * j:3 * j + 3][None, :, :] - at[:, None, :]
        sa = image_shift(da, box)
        per_pair, per_mol = ((da + sa) ** 2).sum(2), ((da + sc[j]) ** 2).sum(2)
        differs = (sa != sc[j]).any(2) & (np.minimum(per_pair, per_mol) < slack_sq)
        if differs.any():
            out.append(int(j))
    return out


# ---- Widom insertion against the oracle --------------------------------------------------------
def widom_oracle_terms(orc, a, com, coords, mol, box, lj_rcut, qq_rcut, alpha=5.6):
    """(d_lj, d_real, d_recip, overlap, (ewald, charges)) of one test molecule mol[12] appended as
    molecule N + 1 to the configuration (com, coords) of the system `a` (topology and tables) in
    the box `box`, kappa = alpha / box.  The reference has no insertion code; dU is defined as the
    change of its potential(..., "ewald") (include/mmc_hip.h):
      d_lj    == orc.lj_poly_du(N+1)
      d_real  == orc.ewald_short(N+1)                   (0 when it reports an overlap)
      d_recip == factor (recip_long(N+1) - recip_long(N)) + orc.ewald_self(the test molecule)
    RecipLong is recomputed from the coordinates, so a wrong S buffer of the device shows."""
    from metropolismontecarlo_amd import structs
    n = com.shape[0]
    L = float(box)
    q3 = np.asarray(a["charge"][:3], dtype=float)
    com1 = np.vstack([com, mol[9:12]])
    coords1 = np.vstack([coords, np.asarray(mol[:9]).reshape(3, 3)])
    first = np.arange(1, 3 * (n + 1), 3, dtype=np.int64)
    at1 = np.concatenate([np.asarray(a["atype"])[:3 * n], np.asarray(a["atype"])[:3]])
    q1 = np.concatenate([np.asarray(a["charge"][:3 * n], dtype=float), q3])
    s1 = orc.System(com1, first, first + 2, coords1, at1, q1, a["eps"], a["sig"], L)
    ew = orc.Ewald(alpha / L, 5, 27, L, factor=structs.factor)
    lj, _ = orc.lj_poly_du(n + 1, s1, lj_rcut)
    real, _, ov = orc.ewald_short(n + 1, s1, ew, qq_rcut)
    rl1 = orc.recip_long(ew, coords1, q1, L)
    rl0 = orc.recip_long(ew, coords, q1[:3 * n], L)
    recip = ew.factor * (rl1 - rl0) + orc.ewald_self(ew, q3)
    return lj, real, recip, ov, (ew, q1)


def widom_close(x, ref):
    """1e-9 K absolute plus 1e-13 of the term (the erfc table's error, tests/test_gpu_table.py)."""
    return abs(x - ref) <= 1e-9 + 1e-13 * abs(ref)


def check_widom(orc, a, b, r, mols, du, ovl, lj_rcut, qq_rcut, alpha=5.6, what=""):
    """Every term and the overlap flag of replica r's insertions mols [M][12] against the oracle, on
    the replica's own coordinates (get_replica) in its own box (get_boxes)."""
    com, coords, _ = b.get_replica(r)
    box = float(b.get_boxes()[r])
    bad = []
    for j in range(mols.shape[0]):
        lj, real, recip, ov, _ = widom_oracle_terms(orc, a, com, coords, mols[j], box, lj_rcut, qq_rcut,
                                                    alpha)
        if bool(ovl[j] & 1) != ov:
            bad.append((j, "overlap", int(ovl[j]), ov))
        for name, x, ref in (("lj", du[j, 0], lj), ("real", du[j, 1], real), ("recip", du[j, 2], recip)):
            if not widom_close(x, ref):
                bad.append((j, name, x, ref))
    assert not bad, f"{what} replica {r}: {bad[:6]}"


def widom_host_sums(du, ovl, boltz0, novl0, temperature):
    """The in-order reduction the library promises, on the host: boltz[r] += exp(-dU / T) of every
    unflagged insertion in insertion order, n_overlap[r] += the flagged ones.  The weight's argument
    is -dU * (1 / T) as k_widom_reduce forms it: with weights of 1e20 and more (|dU| / T ~ 50), the
    rounding of dividing instead moves a weight by 1e-14 of itself.  (Vectorised over the replicas,
    sequential over the insertions: each replica's additions are those of a plain loop.)"""
    bs = np.array(boltz0, dtype=float).copy()
    no = np.array(novl0, dtype=np.int64).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        d = (du[:, :, 0] + du[:, :, 1]) + du[:, :, 2]
        w = np.exp(-d * (1.0 / temperature))
    flagged = ovl != 0
    for j in range(du.shape[1]):
        bs = np.where(flagged[:, j], bs, bs + w[:, j])
    no += flagged.sum(1)
    return bs, no


class _UnreachableLibrary:
    """Stands where a wrapper's library handle does: any call through it fails the test."""

    def __getattr__(self, name):
        def reached(*args):
            raise AssertionError("the library was reached")
        return reached


def fake_batch(method_name, R=2, n_mol=10, **attrs):
    """An object with device.Batch's `method_name` (several names: separate them with blanks) bound
    to it and the attributes the wrappers read: R, n_mol, _h = None, and an _L that fails the test
    when a wrapper's own argument checks let a call through.  `attrs` adds or replaces attributes,
    _L among them.  Needs no built library."""
    from metropolismontecarlo_amd.device import Batch

    class Fake:
        pass
    fake = Fake()
    fake.__dict__.update(dict(R=R, n_mol=n_mol, _h=None, _L=_UnreachableLibrary()), **attrs)
    for name in method_name.split():
        setattr(fake, name, getattr(Batch, name).__get__(fake))
    return fake
