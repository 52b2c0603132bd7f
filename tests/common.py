"""Shared helpers for the tests: load the committed fixtures and build matching inputs for the
oracle (oracle.oracle.System / Ewald) and for the product (numpy arrays for device.Context)."""
import json
import os
import re

import numpy as np

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


# ---- which replica k_move_eval_wave runs where ----------------------------------------------------
def _wave_consts():
    """(waves per workgroup, waves per SIMD) of k_move_eval_wave, read from its source so that the
    unit -> wave map below follows the kernel."""
    src = open(os.path.join(HERE, "..", "metropolismontecarlo_amd", "csrc", "mmc_wave.hpp")).read()
    assert re.search(r"#define WV_MWAVES WV_WAVES\b", src)
    return (int(re.search(r"#define WV_WAVES (\d+)", src).group(1)),
            int(re.search(r"#define WV_OCC (\d+)", src).group(1)))


def wave_units(n_units, wave_wgs=0, n_cus=256):
    """The units each wave of one k_move_eval_wave launch over n_units takes, in the order it takes
    them: the launch has ceil(n_units / WV_MWAVES) workgroups, capped at option "wave_wgs" or at
    4 * WV_OCC / WV_MWAVES per compute unit (mmc_batch.inc), and wave w of workgroup g loops over
    units g * WV_MWAVES + w, + wgs * WV_MWAVES, ... (mmc_wave.hpp).  Lists in wave order."""
    mw, occ = _wave_consts()
    cap = wave_wgs if wave_wgs > 0 else 4 * occ // mw * n_cus
    wgs = min(-(-n_units // mw), cap)
    return [list(range(g * mw + w, n_units, wgs * mw)) for g in range(wgs) for w in range(mw)]


def replicas_by_wave_position(R, n_groups, wave_wgs=0, n_cus=256, parts=1):
    """{local replica: where its unit runs} for the replicas worth checking when a wave runs several
    units: in every group (replicas [R g / G, R (g + 1) / G), mmc_engine.inc) the first, second,
    middle and last unit of wave 0 (which runs the most), the last unit of a wave that runs one unit
    fewer, and the group's first and last replica."""
    out = {}
    for g in range(n_groups):
        r0, r1 = R * g // n_groups, R * (g + 1) // n_groups
        waves = wave_units((r1 - r0) * parts, wave_wgs, n_cus)
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
