"""CPU tests of how device.Batch's wrappers make, accept and pass on their output arrays, without a
library: a recording stand-in takes every call.  One table (CASES) states, per wrapper and option
combination, the outputs by name -> (shape, dtype, position of the pointer in the C call) from the
docstrings and the parameter order of include/mmc_hip.h, the scalar arguments by position, and how
a caller hands arrays back in."""
import collections
import ctypes as C
import itertools
import math
import tracemalloc
import types

import numpy as np
import pytest

from metropolismontecarlo_amd import _lib
from common import fake_batch

R, N = 2, 10
F8, I8, I4, U8, U2, U1 = np.float64, np.int64, np.int32, np.uint64, np.uint16, np.uint8
MASK64 = 2 ** 64 - 1
SEED = 2 ** 64 + 5          # the wrappers pass seed & (2^64 - 1) = 5


class Recorder:
    """Stands for the library: every function records (name, positional arguments), returns 0 = MMC_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def cosd(t):
    return math.cos(math.radians(t))


# ---- the table --------------------------------------------------------------------------------------
# method, fn: the Batch method and the C function it calls.  args, kw: the call.  outs: name ->
# (shape, dtype, position).  null: positions of outputs not asked for (must be None).  scalars:
# position -> value.  inputs: position -> array the pointer there must hold.  ret: how the result
# names its arrays: None = a dict, a str = one array, a tuple = one name per element ("*": a dict).
# give: how arrays come back in: "out" (one array), "out{}" (a dict under out=), "sums" (a dict under
# sums=), "kw" (one keyword each); given: the names that can be handed back (None = all of outs).
Case = collections.namedtuple("Case", "id method fn args kw outs null scalars inputs ret give given attrs")


def case(id, method, fn, args, kw, outs, scalars, null=(), inputs=None, ret=None, give="out{}", given=None,
         attrs=None):
    return Case(id, method, fn, tuple(args), dict(kw), outs, tuple(null), scalars, inputs or {}, ret, give,
                tuple(outs) if given is None else tuple(given), attrs or {})


def flags(*names):
    """Every on/off combination of the named options: (id suffix, dict) pairs."""
    for bits in itertools.product((False, True), repeat=len(names)):
        on = [n for n, b in zip(names, bits) if b]
        yield ("-" + "-".join(on) if on else ""), dict(zip(names, bits))


def solute(S, base):
    return types.SimpleNamespace(n_sites=S, offsets=np.arange(3.0 * S).reshape(S, 3) + base,
                                 charge=np.arange(1.0 * S) + base + 0.25, eps=np.arange(2.0 * S) + base + 0.5,
                                 sig=np.arange(2.0 * S) + base + 0.75)


def cases():
    M, K = 3, 2
    acc = {"boltz_sum": ((R,), F8), "n_overlap": ((R,), I8)}
    off = np.arange(9.0).reshape(3, 3)

    # -- widom family: boltz_sum / n_overlap accumulate; outputs=True adds mol, du, ovl
    for sfx, o in flags("outputs"):
        outs = {"boltz_sum": ((R,), F8, 6), "n_overlap": ((R,), I8, 7)}
        if o["outputs"]:
            outs.update(mol=((R, M, 12), F8, 8), du=((R, M, 3), F8, 9), ovl=((R, M), U1, 10))
        yield case("widom" + sfx, "widom", "mmc_batch_widom", (M, 298.15, SEED), dict(draw0=7, **o), outs,
                   {0: None, 1: M, 2: 5, 3: 7, 5: 298.15}, null=() if o["outputs"] else (8, 9, 10),
                   inputs={4: off}, ret=tuple(outs), give="kw", given=acc, attrs=dict(widom_offsets=off))
    mol = np.arange(R * M * 12.0).reshape(R, M, 12)
    yield case("widom_at", "widom_at", "mmc_batch_widom_at", (mol, 298.15), {},
               {"boltz_sum": ((R,), F8, 4), "n_overlap": ((R,), I8, 5), "du": ((R, M, 3), F8, 6),
                "ovl": ((R, M), U1, 7)}, {0: None, 1: M, 3: 298.15}, inputs={2: mol},
               ret=("boltz_sum", "n_overlap", "du", "ovl"), give="kw", given=acc)
    s = solute(2, 0.0)
    for sfx, o in flags("outputs"):
        outs = {"boltz_sum": ((R,), F8, 10), "n_overlap": ((R,), I8, 11)}
        if o["outputs"]:
            outs.update(mol=((R, M, 3, 3), F8, 12), du=((R, M, 3), F8, 13), ovl=((R, M), U1, 14))
        yield case("widom_solute" + sfx, "widom_solute", "mmc_batch_widom_solute", (s, M, 298.15, SEED),
                   dict(draw0=7, **o), outs, {0: None, 1: 2, 6: M, 7: 5, 8: 7, 9: 298.15},
                   null=() if o["outputs"] else (12, 13, 14), inputs={2: s.offsets, 3: s.charge, 4: s.eps, 5: s.sig},
                   ret=tuple(outs), give="kw", given=acc)
    mol = np.arange(R * M * 9.0).reshape(R, M, 3, 3)
    yield case("widom_solute_at", "widom_solute_at", "mmc_batch_widom_solute_at", (s, mol, 298.15), {},
               {"boltz_sum": ((R,), F8, 8), "n_overlap": ((R,), I8, 9), "du": ((R, M, 3), F8, 10),
                "ovl": ((R, M), U1, 11)}, {0: None, 1: 2, 5: M, 7: 298.15},
               inputs={2: s.charge, 3: s.eps, 4: s.sig, 6: mol}, ret=("boltz_sum", "n_overlap", "du", "ovl"),
               give="kw", given=acc)

    # -- widom_pair: the six sums under sums=; S_A = 2, S_B = 1, K = 2 separations
    a, b = solute(2, 0.0), solute(1, 100.0)
    pair = types.SimpleNamespace(a=a, b=b, eps_ab=np.array([[1.0], [2.0]]), sig_ab=np.array([[3.0], [4.0]]))
    d = np.array([3.0, 4.5])
    six = ("boltz_a", "n_zero_a", "boltz_b", "n_zero_b", "boltz_ab", "n_zero_ab")

    def sums(p0):
        return {"boltz_a": ((R,), F8, p0), "n_zero_a": ((R,), I8, p0 + 1), "boltz_b": ((R, K), F8, p0 + 2),
                "n_zero_b": ((R, K), I8, p0 + 3), "boltz_ab": ((R, K), F8, p0 + 4), "n_zero_ab": ((R, K), I8, p0 + 5)}
    for sfx, o in flags("outputs"):
        outs = sums(19)
        if o["outputs"]:
            outs.update(mol_a=((R, M, 3, 3), F8, 25), mol_b=((R, M, K, 2, 3), F8, 26),
                        du=((R, M, 1 + 2 * K, 3), F8, 27), flags=((R, M, 1 + K), U1, 28))
        yield case("widom_pair" + sfx, "widom_pair pair_sums", "mmc_batch_widom_pair", (pair, d, M, 298.15, SEED),
                   dict(draw0=7, **o), outs, {0: None, 1: 2, 6: 1, 13: K, 15: M, 16: 5, 17: 7, 18: 298.15},
                   null=() if o["outputs"] else (25, 26, 27, 28),
                   inputs={2: a.offsets, 3: a.charge, 4: a.eps, 5: a.sig, 7: b.offsets, 8: b.charge, 9: b.eps,
                           10: b.sig, 11: pair.eps_ab, 12: pair.sig_ab, 14: d},
                   ret=("*", "mol_a", "mol_b", "du", "flags") if o["outputs"] else None, give="sums", given=six)
    mol_a = np.arange(R * M * 9.0).reshape(R, M, 3, 3)
    mol_b = np.arange(R * M * K * 6.0).reshape(R, M, K, 2, 3)
    outs = sums(16)
    outs.update(du=((R, M, 1 + 2 * K, 3), F8, 22), flags=((R, M, 1 + K), U1, 23))
    yield case("widom_pair_at", "widom_pair_at pair_sums", "mmc_batch_widom_pair_at", (pair, mol_a, mol_b, 298.15),
               {}, outs, {0: None, 1: 2, 5: 1, 11: K, 12: M, 15: 298.15},
               inputs={2: a.charge, 3: a.eps, 4: a.sig, 6: b.charge, 7: b.eps, 8: b.sig, 9: pair.eps_ab,
                       10: pair.sig_ab, 13: mol_a, 14: mol_b}, ret=("*", "du", "flags"), give="sums", given=six)
    yield case("pair_sums", "pair_sums", None, (None, K), {}, {k: v[:2] + (None,) for k, v in sums(0).items()}, {},
               give="sums*", given=six)

    # -- deletion: sel of 3 molecules, bins = (5, ...) -> 7 slots
    sel = np.array([4, 0, 4])
    for sfx, o in flags("bins", "per_replica", "details"):
        if o["per_replica"] and not o["bins"]:
            continue                       # per_replica only shapes the histogram
        outs = {"esum": ((R, 4), F8, 9), "boltz_sum": ((R,), F8, 10), "n_flagged": ((R,), I8, 11)}
        null = []
        if o["bins"]:
            outs["hist"] = ((R, 7) if o["per_replica"] else (7,), U8, 8)
        else:
            null.append(8)
        if o["details"]:
            outs.update(du=((R, 3, 3), F8, 12), ovl=((R, 3), U1, 13))
        else:
            null += [12, 13]
        bins = (5, -100.0, 50.0) if o["bins"] else None
        yield case("deletion" + sfx, "deletion", "mmc_batch_deletion", (298.15,),
                   dict(sel=sel, bins=bins, per_replica=o["per_replica"], details=o["details"]), outs,
                   {0: None, 1: 3, 3: 298.15, 4: 5 if bins else 0, 5: -100.0 if bins else 0.0,
                    6: 50.0 if bins else 0.0, 7: int(o["per_replica"])}, null=null, inputs={2: sel.astype(I4)},
                   give="kw", given=("boltz_sum", "n_flagged"))
    yield case("deletion-all", "deletion", "mmc_batch_deletion", (298.15,), {},
               {"esum": ((R, 4), F8, 9), "boltz_sum": ((R,), F8, 10), "n_flagged": ((R,), I8, 11)},
               {0: None, 1: N, 2: None, 3: 298.15, 4: 0, 5: 0.0, 6: 0.0, 7: 0}, null=(8, 12, 13), give="kw",
               given=("boltz_sum", "n_flagged"))

    # -- forces
    mass = np.array([15.9994, 1.00794, 1.00794])
    for sfx, o in flags("details"):
        outs = {"fsum": ((R, 9), F8, 8), "n_flagged": ((R,), I8, 9)}
        if o["details"]:
            outs.update(force=((R, 3, 3), F8, 4), torque=((R, 3, 3), F8, 5), vir=((R, 3, 3), F8, 6),
                        atom=((R, 3, 3, 3), F8, 7), ovl=((R, 3), U1, 10))
        yield case("forces" + sfx, "forces", "mmc_batch_forces", (), dict(sel=sel, mass=mass, **o), outs,
                   {0: None, 1: 3}, null=() if o["details"] else (4, 5, 6, 7, 10),
                   inputs={2: sel.astype(I4), 3: mass}, give="kw", given=("n_flagged",))
    yield case("forces-all", "forces", "mmc_batch_forces", (), {},
               {"fsum": ((R, 9), F8, 8), "n_flagged": ((R,), I8, 9)}, {0: None, 1: N, 2: None, 3: None},
               null=(4, 5, 6, 7, 10), give="kw", given=("n_flagged",))

    # -- the single-array wrappers
    for sfx, o in flags("per_replica"):
        lead, per = ((R,) if o["per_replica"] else ()), int(o["per_replica"])
        yield case("rdf_sites" + sfx, "rdf_sites", "mmc_batch_rdf_sites", (7,), dict(r_max=9.5, **o),
                   {"out": (lead + (6, 8), U8, 4)}, {0: None, 1: 7, 2: 9.5, 3: per}, ret="out", give="out")
        yield case("orient_corr" + sfx, "orient_corr", "mmc_batch_orient_corr", (7,), dict(r_max=9.5, **o),
                   {"out": (lead + (4, 9), I8, 4)}, {0: None, 1: 7, 2: 9.5, 3: per}, ret="out", give="out")
        # n_max = 3: 10 shells; int64 [R, 6, S] at 4 with per_replica, else float64 [6, S] at 5
        yield case("structure_factor" + sfx, "structure_factor", "mmc_batch_structure_factor", (3,), o,
                   {"count": ((10,), I4, 3), "out": ((R, 6, 10), I8, 4) if per else ((6, 10), F8, 5)},
                   {0: None, 1: 3, 2: per}, null=(5,) if per else (4,), ret=("count", "out"), give="out",
                   given=("out",))
    yield case("dipoles", "dipoles", "mmc_batch_dipoles", (), {}, {"out": ((R, 3), F8, 1)}, {0: None}, ret="out",
               give="out")

    # -- pair_energy: uhist only with n_ebins != 0, nhb only with u_hb; flagged (1,) or (R,)
    for sfx, o in flags("per_replica", "ebins", "hb"):
        lead, per = ((R,) if o["per_replica"] else ()), int(o["per_replica"])
        outs = {"rows": (lead + (3, 9), I8, 8), "flagged": (lead if per else (1,), U8, 11)}
        null = []
        if o["ebins"]:
            outs["uhist"] = (lead + (6,), U8, 9)
        else:
            null.append(9)
        if o["hb"]:
            outs["nhb"] = (lead + (9,), U8, 10)
        else:
            null.append(10)
        yield case("pair_energy" + sfx, "pair_energy", "mmc_batch_pair_energy", (7,),
                   dict(r_max=9.5, n_ebins=4 if o["ebins"] else 0, u_lo=-3000.0, u_hi=1500.0,
                        u_hb=-1132.2 if o["hb"] else None, per_replica=o["per_replica"]), outs,
                   {0: None, 1: 7, 2: 9.5, 3: 4 if o["ebins"] else 0, 4: -3000.0, 5: 1500.0,
                    6: -1132.2 if o["hb"] else 0.0, 7: per}, null=null, ret="namedtuple")

    # -- the per-molecule observables: histograms [R, ...] with per_replica, details adds per-molecule arrays
    for sfx, o in flags("per_replica", "details"):
        lead, per, det = ((R,) if o["per_replica"] else ()), int(o["per_replica"]), o["details"]

        outs = {"hb_hist": (lead + (3, 9), U8, 5), "q_hist": (lead + (6,), U8, 6), "q_sum": ((R, 2), F8, 7)}
        if det:
            outs.update(nbr=((R, N, 4), I4, 8), q=((R, N), F8, 9), hb=((R, N, 2), U1, 10))
        yield case("local_order" + sfx, "local_order", "mmc_batch_local_order", (), dict(q_bins=6, r_hb=3.4,
                   theta_deg=25.0, **o), outs, {0: None, 1: 3.4, 2: cosd(25.0), 3: 6, 4: per},
                   null=() if det else (8, 9, 10))

        outs = {"rank_hist": (lead + (3, 5), U8, 15), "lsi_hist": (lead + (6,), U8, 16),
                "ang_hist": (lead + (7,), U8, 17), "zeta_hist": (lead + (8,), U8, 18), "flagged": ((R,), U8, 19),
                "sums": ((R, 4), F8, 20)}
        if det:
            outs.update(count=((R, N), I4, 21), nbr=((R, N, 16), I4, 22), lsi=((R, N), F8, 23),
                        zeta=((R, N), F8, 24))
        yield case("shell_order" + sfx, "shell_order", "mmc_batch_shell_order", (),
                   dict(r_list=6.1, r_lsi=3.6, r_ang=3.2, r_hb=3.4, theta_deg=25.0, n_rank=3, r_bins=4, lsi_bins=5,
                        lsi_max=0.3, ang_bins=6, zeta_bins=7, zeta_lo=-1.25, zeta_hi=2.25, **o), outs,
                   {0: None, 1: 6.1, 2: 3.6, 3: 3.2, 4: 3.4, 5: cosd(25.0), 6: 3, 7: 4, 8: 5, 9: 0.3, 10: 6, 11: 7,
                    12: -1.25, 13: 2.25, 14: per}, null=() if det else (21, 22, 23, 24))

        outs = {"vol_hist": (lead + (4,), U8, 9), "eta_hist": (lead + (5,), U8, 10),
                "face_hist": (lead + (65,), U8, 11), "side_hist": (lead + (17,), U8, 12),
                "nbr_hist": (lead + (6,), U8, 13), "flagged": ((R, 3), U8, 14), "sums": ((R, 8), F8, 15)}
        if det:
            outs.update(vol=((R, N), F8, 16), area=((R, N), F8, 17), faces=((R, N), I4, 18),
                        nbr=((R, N, 64), I4, 19), face_area=((R, N, 64), F8, 20))
        yield case("voronoi" + sfx, "voronoi", "mmc_batch_voronoi", (),
                   dict(r_list=6.5, area_min=0.125, v_bins=3, v_max=70.0, eta_bins=4, eta_max=2.5, r_bins=5, **o),
                   outs, {0: None, 1: 6.5, 2: 0.125, 3: 3, 4: 70.0, 5: 4, 6: 2.5, 7: 5, 8: per},
                   null=() if det else (16, 17, 18, 19, 20))

        outs = {"q_hist": (lead + (4,), U8, 13), "qbar_hist": (lead + (4,), U8, 14), "c_hist": (lead + (6,), U8, 15),
                "ab_hist": (lead + (17, 17), U8, 16), "size_hist": (lead + (N + 1,), U8, 17),
                "stats": ((R, 8), I8, 18), "sums": ((R, 4), F8, 19)}
        if det:
            outs.update(q=((R, N), F8, 20), qbar=((R, N), F8, 21), nbr=((R, N, 16), I4, 22), ab=((R, N, 2), U1, 23),
                        label=((R, N), I4, 24))
        yield case("bond_order" + sfx, "bond_order", "mmc_batch_bond_order", (),
                   dict(l=6, r_nb=3.4, n_nb=5, a=(-np.inf, -0.75), b=(-0.3, 0.2), min_a=2, min_ab=3, q_bins=3,
                        c_bins=5, **o), outs,
                   {0: None, 1: 6, 2: 3.4, 3: 5, 4: -math.inf, 5: -0.75, 6: -0.3, 7: 0.2, 8: 2, 9: 3, 10: 3, 11: 5,
                    12: per}, null=() if det else (20, 21, 22, 23, 24))

        # three criteria, the scalars broadcast
        outs = {"size_hist": (lead + (3, N + 1), U8, 6), "deg_hist": (lead + (3, 17), U8, 7),
                "stats": ((R, 3, 8), I8, 8)}
        if det:
            outs.update(label=((R, 3, N), I4, 9), nbr=((R, 3, N, 16), I4, 10))
        yield case("hbond_network" + sfx, "hbond_network", "mmc_batch_hbond_network", (),
                   dict(r_hb=(3.3, 3.5, 3.7), theta_deg=30.0, min_bonds=(0, 1, 2), **o), outs, {0: None, 1: 3, 5: per},
                   null=() if det else (9, 10),
                   inputs={2: np.array([3.3, 3.5, 3.7]), 3: np.full(3, cosd(30.0)), 4: np.array([0, 1, 2], dtype=I4)})

        # ring only with details and max_rings > 0; count is uint16
        for mr in (0, 5):
            outs = {"ring_hist": (lead + (3, 9), U8, 5), "member_hist": (lead + (9, 33), U8, 6),
                    "stats": ((R, 8), I8, 7)}
            null = []
            if det:
                outs["count"] = ((R, N, 9), U2, 8)
            else:
                null.append(8)
            if det and mr:
                outs["ring"] = ((R, mr, 8), I4, 10)
            else:
                null.append(10)
            yield case(f"hbond_rings{sfx}-max_rings{mr}", "hbond_rings", "mmc_batch_hbond_rings", (),
                       dict(r_hb=3.4, theta_deg=25.0, n_max=7, max_rings=mr, **o), outs,
                       {0: None, 1: 3.4, 2: cosd(25.0), 3: 7, 4: per, 9: mr}, null=null)

    # -- cavity / cavity_at: P = 4 points, K = 2 radii, n_cap = 5, nn_hist only with nn_bins > 0
    rad = np.array([2.5, 3.5])
    pts = np.arange(R * 4 * 3.0).reshape(R, 4, 3)
    for sfx, o in flags("per_replica", "details", "nn"):
        lead, per, det = ((R,) if o["per_replica"] else ()), int(o["per_replica"]), o["details"]
        kw = dict(radii=rad, site=-1, n_cap=5, nn_bins=3 if o["nn"] else 0, nn_max=6.0 if o["nn"] else None,
                  per_replica=o["per_replica"], details=det)
        for at in (False, True):
            p0 = 10 if at else 11          # occ_hist; cavity has seed, draw0 in front and points_out behind
            outs = {"occ_hist": (lead + (2, 6), U8, p0), "occ_mom": (lead + (2, 2), U8, p0 + 1)}
            null = []
            if o["nn"]:
                outs["nn_hist"] = (lead + (4,), U8, p0 + 2)
            else:
                null.append(p0 + 2)
            tail = p0 + 3 if at else p0 + 4
            if det:
                outs["points"] = ((R, 4, 3), F8, 2 if at else 14)
                outs.update(count=((R, 4, 2), I4, tail), nn_r2=((R, 4), F8, tail + 1), nn_idx=((R, 4), I4, tail + 2))
            else:
                null += [tail, tail + 1, tail + 2] + ([] if at else [14])
            common = {0: None, 1: 4, p0 - 7: -1, p0 - 6: 2, p0 - 4: 5, p0 - 3: 3 if o["nn"] else 0,
                      p0 - 2: 6.0 if o["nn"] else 0.0, p0 - 1: per}
            if at:
                yield case("cavity_at" + sfx, "cavity_at _cavity", "mmc_batch_cavity_at", (pts,), kw, outs, common,
                           null=null, inputs={5: rad} if det else {2: pts, 5: rad}, give=None, given=())
            else:
                yield case("cavity" + sfx, "cavity _cavity", "mmc_batch_cavity", (4, SEED), dict(draw0=7, **kw), outs,
                           {**common, 2: 5, 3: 7}, null=null, inputs={6: rad}, give=None, given=())

    # -- volume_perturb: K = 3 scales
    sc = np.array([0.99, 1.0, 1.01])
    for sfx, o in flags("details"):
        outs = {"boltz_sum": ((R, 3), F8, 4), "n_overlap": ((R, 3), I8, 5)}
        if o["details"]:
            outs.update(du=((R, 3, 4), F8, 6), base=((R, 4), F8, 7))
        yield case("volume_perturb" + sfx, "volume_perturb", "mmc_batch_volume_perturb", (298.15,),
                   dict(scales=sc, **o), outs, {0: None, 1: 3, 3: 298.15}, null=() if o["details"] else (6, 7),
                   inputs={2: sc}, ret=tuple(outs), give="kw", given=("boltz_sum", "n_overlap"))


CASES = list(cases())
GIVING = [(c, name) for c in CASES for name in c.given]


def run(c, **more):
    rec = Recorder()
    b = fake_batch(c.method, R=R, n_mol=N, _L=rec, box=20.0, **c.attrs)
    result = getattr(b, c.method.split()[0])(*c.args, **dict(c.kw, **more))
    return result, rec


def arrays(c, result):
    """name -> array of a wrapper's result, by the case's `ret`."""
    if c.ret is None:
        return dict(result)
    if c.ret == "namedtuple":
        return {k: v for k, v in result._asdict().items() if v is not None}
    if isinstance(c.ret, str):
        return {c.ret: result}
    got = {}
    for name, v in zip(c.ret, result):
        got.update(v if name == "*" else {name: v})
    assert len(result) == len(c.ret)
    return got


def give_back(c, arrs):
    """The keywords that hand `arrs` (name -> array) back to the wrapper."""
    if c.give == "out":
        return dict(out=arrs["out"])
    if c.give == "out{}":
        return dict(out=dict(arrs))
    if c.give == "sums":
        return dict(sums=dict(arrs))
    assert c.give == "kw"
    return dict(arrs)


def address(arg):
    return C.cast(arg, C.c_void_p).value


@pytest.mark.parametrize("c", [c for c in CASES if c.fn], ids=lambda c: c.id)
def test_outputs_are_made_to_the_documented_shapes_and_passed_at_their_positions(c):
    result, rec = run(c)
    got = arrays(c, result)
    assert set(got) == set(c.outs)
    (fn, args), = rec.calls
    want_types = _lib.SIGNATURES[c.fn]
    assert fn == c.fn and len(args) == len(want_types)
    for name, (shape, dt, pos) in c.outs.items():
        a = got[name]
        assert isinstance(a, np.ndarray) and a.shape == shape and a.dtype == dt and a.flags.c_contiguous, name
        if not (name == "points" and "cavity_at" in c.method):     # the caller's own points come back
            assert not a.any(), name
        assert type(args[pos]) is want_types[pos], name     # the pointer class the binding declares
        assert address(args[pos]) == a.ctypes.data, name
    for pos in c.null:
        assert args[pos] is None, pos
    for pos, v in c.scalars.items():
        assert args[pos] == (pytest.approx(v, abs=1e-15) if isinstance(v, float) else v), pos
        assert v is None or type(args[pos]) is type(v), pos
    for pos, v in c.inputs.items():
        assert type(args[pos]) is want_types[pos], pos
        seen = np.ctypeslib.as_array(args[pos], shape=v.shape)
        assert seen.dtype == v.dtype and np.allclose(seen, v, rtol=0, atol=1e-15), pos
    # every position is accounted for
    assert sorted([p for _, _, p in c.outs.values()] + list(c.null) + list(c.scalars) + list(c.inputs)) \
        == list(range(len(args)))


@pytest.mark.parametrize("c", [c for c in CASES if c.given], ids=lambda c: c.id)
def test_arrays_handed_back_are_returned_by_identity_and_passed_on(c):
    if c.give == "sums*":                                    # pair_sums itself: no library call
        first = fake_batch("pair_sums", R=R, n_mol=N).pair_sums(*c.args)
        again = fake_batch("pair_sums", R=R, n_mol=N).pair_sums(first, c.args[1])
        assert set(first) == set(c.outs) and all(again[k] is first[k] for k in first)
        for name, (shape, dt, _) in c.outs.items():
            assert first[name].shape == shape and first[name].dtype == dt and not first[name].any()
        return
    first = arrays(c, run(c)[0])
    given = {k: first[k] for k in c.given}
    result, rec = run(c, **give_back(c, given))
    again = arrays(c, result)
    (_, args), = rec.calls
    for name in c.given:
        assert again[name] is first[name], name
        assert address(args[c.outs[name][2]]) == first[name].ctypes.data, name
    for name in set(c.outs) - set(c.given):
        assert again[name] is not first[name], name


def bad_versions(shape, dt):
    """(what, stand-in) for an array of (shape, dt) that a wrapper must refuse."""
    yield "dtype", np.zeros(shape, dtype=np.float32 if dt == np.float64 else np.float64)
    yield "shape", np.zeros(shape[:-1] + (shape[-1] + 1,), dtype=dt)
    yield "rank", np.zeros(shape + (1,), dtype=dt)
    strided = np.zeros(shape[:-1] + (2 * shape[-1],), dtype=dt)[..., ::2]
    assert strided.shape == shape
    if not strided.flags.c_contiguous:                       # (one element is contiguous whatever its stride)
        yield "strided", strided
    yield "list", np.zeros(shape, dtype=dt).tolist()


@pytest.mark.parametrize("c,name", GIVING, ids=lambda v: v if isinstance(v, str) else v.id)
def test_an_array_of_the_wrong_kind_is_refused_before_the_library(c, name):
    shape, dt, _ = c.outs[name]
    for what, bad in bad_versions(shape, dt):
        if c.give == "sums*":
            with pytest.raises(ValueError):
                fake_batch("pair_sums", R=R, n_mol=N).pair_sums({name: bad}, c.args[1])
            continue
        rec = Recorder()
        b = fake_batch(c.method, R=R, n_mol=N, _L=rec, box=20.0, **c.attrs)
        with pytest.raises(ValueError):
            getattr(b, c.method.split()[0])(*c.args, **dict(c.kw, **give_back(c, {name: bad})))
        assert rec.calls == [], what


DICT_WRAPPERS = list({c.method: c for c in reversed(CASES) if c.give == "out{}"}.values())   # each one's plainest case


@pytest.mark.parametrize("c", DICT_WRAPPERS, ids=lambda c: c.id)
def test_unknown_keys_in_out(c):
    """pair_energy refuses a key that is no output of the call; the other six ignore it."""
    extra = dict(out=dict(no_such_output=np.zeros(3)))
    if c.method == "pair_energy":
        rec = Recorder()
        with pytest.raises(ValueError):
            fake_batch(c.method, R=R, n_mol=N, _L=rec).pair_energy(*c.args, **dict(c.kw, **extra))
        with pytest.raises(ValueError):      # uhist is no output without energy bins
            fake_batch(c.method, R=R, n_mol=N, _L=rec).pair_energy(7, out=dict(uhist=np.zeros(6, dtype=U8)))
        assert rec.calls == []
    else:
        result, rec = run(c, **extra)
        assert set(result) == set(c.outs) and len(rec.calls) == 1


@pytest.mark.parametrize("c", DICT_WRAPPERS, ids=lambda c: c.id)
def test_an_out_that_is_no_dict_is_refused(c):
    """By a ValueError, in all seven alike, before the library is called."""
    rec = Recorder()
    b = fake_batch(c.method, R=R, n_mol=N, _L=rec)
    with pytest.raises(ValueError):
        getattr(b, c.method)(*c.args, **dict(c.kw, out=[np.zeros(3)]))
    assert rec.calls == []


def test_the_seven_dict_wrappers_are_all_in_the_table():
    assert sorted(c.method for c in DICT_WRAPPERS) == ["bond_order", "hbond_network", "hbond_rings", "local_order",
                                                       "pair_energy", "shell_order", "voronoi"]


def test_sizes_the_library_refuses_still_get_arrays_and_the_raw_value_is_passed():
    rec = Recorder()
    out = fake_batch("rdf_sites", _L=rec).rdf_sites(-3, per_replica=True)
    assert out.shape == (R, 6, 1) and rec.calls[0][1][1] == -3
    res = fake_batch("pair_energy", _L=rec).pair_energy(-3, n_ebins=-4)
    assert res.rows.shape == (3, 2) and res.uhist.shape == (2,) and rec.calls[1][1][1] == -3 and rec.calls[1][1][3] == -4
    res = fake_batch("deletion", _L=rec).deletion(298.15, bins=(-5, 0.0, 1.0))
    assert res["hist"].shape == (2,) and rec.calls[2][1][4] == -5


@pytest.mark.parametrize("per", [False, True])
def test_sdf_returns_views_of_the_library_layout(per):
    # fold 3, n_half 2: 2 x 2 x 4 cells + outside + noframe
    lead = (R,) if per else ()
    rec = Recorder()
    b = fake_batch("sdf", R=R, n_mol=N, _L=rec)
    res = b.sdf(2, 0.5, fold=3, site_mask=5, per_replica=per)
    assert res.grid.shape == lead + (2, 2, 4) and res.outside.shape == lead and res.noframe.shape == lead
    assert res.grid.dtype == res.outside.dtype == res.noframe.dtype == U8 and not res.grid.any()
    (fn, args), = rec.calls
    assert fn == "mmc_batch_sdf" and args[:6] == (None, 2, 0.5, 3, 5, int(per))
    assert type(args[6]) is _lib.SIGNATURES[fn][6] and address(args[6]) == res.grid.ctypes.data
    out = np.zeros(lead + (18,), dtype=U8)
    res = b.sdf(2, 0.5, per_replica=per, out=out)
    assert address(rec.calls[1][1][6]) == out.ctypes.data
    out[..., 0], out[..., 16], out[..., 17] = 3, 4, 5
    assert (res.grid[..., 0, 0, 0] == 3).all() and (res.outside == 4).all() and (res.noframe == 5).all()
    for what, bad in bad_versions(lead + (18,), U8):
        with pytest.raises(ValueError):
            b.sdf(2, 0.5, per_replica=per, out=bad)
    assert len(rec.calls) == 2


def test_sdf_allocates_two_slots_for_a_grid_the_library_refuses():
    """More than 32768 cells and no `out`: the library gets a pointer to refuse, not 300 kB of zeros."""
    class Refused(Exception):
        pass

    class Refusing:
        @staticmethod
        def mmc_batch_sdf(*args):
            assert args[6] is not None
            raise Refused
    b = fake_batch("sdf", R=R, n_mol=N, _L=Refusing)
    tracemalloc.start()
    try:
        with pytest.raises(Refused):
            b.sdf(17, 0.5, fold=0)                           # 34^3 = 39304 cells
        assert tracemalloc.get_traced_memory()[1] < 34 ** 3 * 8 // 4
    finally:
        tracemalloc.stop()
    with pytest.raises(ValueError):                          # a caller's array is still held to the full shape
        b.sdf(17, 0.5, fold=0, out=np.zeros(2, dtype=U8))


def test_cavity_refusals_and_the_callers_points():
    rec = Recorder()
    b = fake_batch("cavity cavity_at _cavity", R=R, n_mol=N, _L=rec)
    with pytest.raises(ValueError):
        b.cavity(4, 1, nn_bins=3)                            # nn_bins > 0 needs nn_max
    with pytest.raises(ValueError):
        b.cavity_at(np.zeros((R, 4, 2)))
    assert rec.calls == []
    pts = np.arange(R * 4 * 3.0).reshape(R, 4, 3)
    assert b.cavity_at(pts, details=True)["points"] is pts
    assert "points" not in b.cavity_at(pts) and "points" not in b.cavity(4, 1)


def test_volume_perturb_takes_dv_for_scales():
    rec = Recorder()
    b = fake_batch("volume_perturb", R=R, n_mol=N, _L=rec, box=20.0)
    with pytest.raises(ValueError):
        b.volume_perturb(298.15)
    with pytest.raises(ValueError):
        b.volume_perturb(298.15, scales=[1.0], dv=[1.0])
    assert rec.calls == []
    b.volume_perturb(298.15, dv=[-80.0, 80.0])
    args = rec.calls[0][1]
    assert args[1] == 2
    assert np.allclose(np.ctypeslib.as_array(args[2], shape=(2,)), [(7920 / 8000) ** (1 / 3), (8080 / 8000) ** (1 / 3)],
                       rtol=1e-15, atol=0)


# ---- the helper itself ------------------------------------------------------------------------------
def helper():
    from metropolismontecarlo_amd import device
    return device


def test_helper_makes_zero_arrays_and_returns_given_ones_by_identity():
    dev = helper()
    spec = {"a": ((2, 3), F8), "b": ((4,), U2)}
    res = dev._outputs(spec, None)
    assert list(res) == ["a", "b"] and res["a"].shape == (2, 3) and res["a"].dtype == F8 and not res["a"].any()
    assert res["b"].shape == (4,) and res["b"].dtype == U2
    again = dev._outputs(spec, {"a": res["a"], "b": None})
    assert again["a"] is res["a"] and again["b"] is not res["b"]
    assert dev._output(res["b"], (4,), U2, "b") is res["b"]
    assert dev._output(None, (4,), U2, "b").shape == (4,)


def test_helper_names_entry_dtype_and_shape_in_its_refusal():
    dev = helper()
    with pytest.raises(ValueError, match=r"out\['a'\].*float64.*\(2, 3\)"):
        dev._outputs({"a": ((2, 3), F8)}, {"a": np.zeros((2, 3), dtype=np.float32)})
    with pytest.raises(ValueError, match=r"n_flagged.*int64.*\(2,\)"):
        dev._output([0, 0], (2,), I8, "n_flagged")
    with pytest.raises(ValueError):
        dev._outputs({"a": ((2, 3), F8)}, [1, 2])
    # unknown keys: ignored, or refused with known_only
    assert list(dev._outputs({"a": ((2,), F8)}, {"zzz": 1})) == ["a"]
    with pytest.raises(ValueError, match="zzz"):
        dev._outputs({"a": ((2,), F8)}, {"zzz": 1}, known_only=True)


def test_helper_pointers_take_their_type_from_the_dtype():
    dev = helper()
    for dt, ct in ((U8, C.c_uint64), (I8, C.c_int64), (F8, C.c_double), (I4, C.c_int32), (U1, C.c_uint8),
                   (U2, C.c_uint16)):
        a = np.zeros(3, dtype=dt)
        p = dev._ptr(a)
        assert type(p) is C.POINTER(ct) and address(p) == a.ctypes.data
    res = {"x": np.zeros(2), "y": np.zeros(2, dtype=I4)}
    px, pz, py = dev._ptrs(res, "x", "z", "y")
    assert pz is None and type(px) is C.POINTER(C.c_double) and type(py) is C.POINTER(C.c_int32)
    assert address(py) == res["y"].ctypes.data
