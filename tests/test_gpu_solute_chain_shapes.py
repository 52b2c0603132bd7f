"""A fixed solute at the launch shapes it ships in (include/mmc_hip.h, "A fixed solute"): every row of
k_solute_move, and the solute's observables beyond one pass of their thread strides.

k_solute_move (mmc_solute_chain.hpp) puts a replica in each row of 16 lanes, four replicas per wave, sixteen
per workgroup.  R = 37 replicas of 65 waters are three workgroups of 16, 16 and 5 live rows and 11 idle ones;
with n_groups = 2 the run plan launches the replicas [0, 18) and [18, 37), two workgroups each, the second
launch with r0 = 18.  Replica r starts from the waters translated rigidly by its own vector and folded back
into the box while the solute stays where it is, so every replica has its own solute energy from step 0.
  B1  chains of 65 device-proposed steps on the wave kernel and the workgroup-per-move kernel, one and two
      groups, against solute_chain_ref.replay of the oracle's N + 1 system for the replicas 0, 5, 21, 31, 36
      (the first row; a row of wave 1; a row of workgroup 1; the last row of workgroup 1; the last live row).
  B2  all 37 chains again as shards of three replicas (replica0 = 3 k, and 34 for the last: a batch of ONE
      replica is another shape, see SHARDS): the chain of replica r depends on (seed, replica0 + r) only, so
      trace, energies, coordinates and S(k) are the same bytes.
  B3  overlaps stay in their row: through mmc_batch_eval, replicas 5, 22 and 36 propose an overlap with the
      dipole's negative site, replica 20 starts in one, and the rows beside them in their waves report none.
The solute's observables at 1090 waters (1024 + 64 + 2: k_hydration_map's 1024 threads make a second pass
of 66 waters, k_rdf_solute's 256 a fifth, k_solute_total's 64 lanes an eighteenth), with waters planted by
index so that both passes of one thread carry tails, and with a water whose energy is flagged though it
does not overlap (methane is uncharged: no overlap rule applies); and one chain beside the wave kernel at
that size, several 64-molecule blocks per scan and the candidate lists in use.

Tolerances are those of test_gpu_solute_chain_paths.py (TOL (|dU| + 1e4) per step, 2e-13 A, 1e-9 on S(k)),
of solute_ref.solute_close and of test_gpu_hydration_map.check_energy_rows; none is new.  Every test prints
the largest deviation it met before it asserts."""
import numpy as np
import pytest

import common
import hydration_map_ref as hm
import solute_chain_ref as scr
import solute_ref as sr
import test_gpu_solute_chain as tsc
from test_gpu_hydration_map import check_energy_rows
from test_gpu_solute_chain_paths import DPHI, DR, LJ, QQ, T, TOL, check_trace, make_batch, proposal_of

pytestmark = pytest.mark.gpu

N, R, STEPS, SEED = 65, 37, 65, 2468
PICKS = (0, 5, 21, 31, 36)
SHAPES = ((2, 1), (2, 2), (1, 1), (1, 2))        # (option "kernel", n_groups)
FORCED = {"accept_on_device": 0, "persistent": 0}  # without a solute: the path a solute takes
# replica0 of the shards of three: 0, 3, ... 33, and 34 -- the replicas 34 and 35 run twice, so that no shard
# is a batch of one replica.  Such a batch builds S(k) and the totals in the one-system kernel
# (DeviceSystem::recip_long_all / totals_ewald, R == 1: k_potential_one), whose sums differ from the batch
# kernels' in the last bits: measured here, replica 36 run alone had the same decisions, energies and
# coordinates but other bytes in 64 or 65 of its 65 dU (by up to 4e-12 K) and in S(k) (by up to 4e-15), on
# both kernels, with the solute and without it.  That is the starting S(k)'s, not the chain's and not the
# solute's; the shape the chain tests hold to the oracle is R = 3.
SHARDS = tuple(range(0, R - 2, 3)) + (R - 3,)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def water():
    return sr.first_molecules(common.nist_arrays(3, "unwrapped"), N)


def starts_around(a, mol, n_rep, seed, clear=2.0):
    """[(com, coords)] of n_rep replicas: the waters of `a` moved rigidly by a vector of the replica's own and
    folded back molecule by molecule, the vector drawn again until every site of the solute `mol` keeps
    `clear` A from every atom and at least three centres of mass lie within 6 A of its reference point (the
    chain starts from a finite energy, and the solute is felt)."""
    rng = np.random.default_rng(seed)
    box, com, at = float(a["box"]), np.asarray(a["com"]), np.asarray(a["coords"]).reshape(-1, 3, 3)
    out = []
    while len(out) < n_rep:
        c = com + rng.random(3) * box
        shift = -box * np.floor(c / box)
        c, x = c + shift, at + (c + shift - com)[:, None, :]
        d = mol[:-1, None, :] - x.reshape(-1, 3)[None, :, :]
        d = d + common.image_shift(d, box)
        g = c - mol[-1]
        g = g + common.image_shift(g, box)
        if (d * d).sum(2).min() > clear ** 2 and ((g * g).sum(1) < 36.0).sum() >= 3:
            out.append((c, x.reshape(-1, 3).copy()))
    return out


def batch_with(a, reps, sol, mol, opts):
    b = tsc.batch_of(a, reps)
    for k, v in opts.items():
        b.set_option(k, v)
    if sol is not None:
        b.set_solute(sol, mol)
    return b


def run_chains(a, reps, sol, mol, opts, n_groups, replica0=0, steps=STEPS, seed=SEED):
    """One call of `steps` steps with the trace on: what the chains leave, replica by replica."""
    with batch_with(a, reps, sol, mol, opts) as b:
        e0 = b.potential_ewald(as_array=True)["energy"].copy()
        b.set_option("trace_steps", steps)
        e1, st = b.run(steps, T, DR, DPHI, seed=seed, energies=e0, n_parts=1, n_groups=n_groups, n_threads=2,
                       replica0=replica0)
        d, f = b.get_trace(steps)
        finals = [b.get_replica(r) for r in range(len(reps))]       # (before anything rebuilds S(k))
        assert st["moves"] == len(reps) * steps and st["device_decisions"] == 0 and st["server_steps"] == 0, st
        cand = b.cand_stats()
        fresh = b.potential_ewald(as_array=True)["energy"].copy()
    return dict(e0=e0, e1=e1, d=d, f=f, finals=finals, cand=cand, fresh=fresh)


class Shapes:
    """The 37-replica system of B1 and B2 with its runs, each made once."""

    def __init__(self, a):
        self.a, self.box = a, float(a["box"])
        self.sol = sr.synthetic(a, 16, seed=7)          # sixteen sites: every lane of a row works
        self.mol = sr.placed(self.sol.offsets, tsc.corner(self.box), sr.rotation(np.random.default_rng(3)))
        self.reps = starts_around(a, self.mol, R, seed=37, clear=2.4)
        self._big, self._shards = {}, {}

    def big(self, kernel, n_groups, solute=True):
        key = (kernel, n_groups, solute)
        if key not in self._big:
            opts = dict(FORCED, device_moves=1, kernel=kernel)
            self._big[key] = run_chains(self.a, self.reps, self.sol if solute else None, self.mol, opts, n_groups)
        return self._big[key]

    def shards(self, kernel, solute=True):
        """The same chains in batches of three replicas, replica0 in SHARDS."""
        key = (kernel, solute)
        if key not in self._shards:
            opts = dict(FORCED, device_moves=1, kernel=kernel)
            self._shards[key] = [run_chains(self.a, self.reps[k:k + 3], self.sol if solute else None, self.mol, opts, 2,
                                            replica0=k) for k in SHARDS]
        return self._shards[key]


@pytest.fixture(scope="module")
def shapes(water):
    return Shapes(water)


@pytest.fixture(scope="module")
def replays(orc, shapes):
    """{r: (trace, sum of the accepted dU, com, coords, fresh S(k), fresh totals)} of the oracle's chains of PICKS."""
    s = shapes
    so = sr.SoluteOracle(orc, s.a, s.sol, LJ, QQ)
    out = {}
    for r in PICKS:
        n1 = scr.N1(so, s.reps[r][0], s.reps[r][1], s.mol, s.box)
        trace, e_acc, _ = scr.replay(n1, proposal_of(SEED, r, s.box), STEPS, T)
        n1.recip_long()
        out[r] = (trace, e_acc, n1.s.com[:-1].copy(), n1.s.coords[:3 * N].copy(), n1.ew.sumQExpOld.copy(), n1.potential())
        n_acc = sum(f & 1 for _, f in trace)
        assert n_acc > 10 and n_acc < STEPS, (r, n_acc)          # the chain moves, and something is rejected
    return out


def test_the_replicas_differ_from_step_0(shapes):
    with batch_with(shapes.a, shapes.reps, shapes.sol, shapes.mol, {}) as b:
        b.recip_long()
        u_lj, u_real, ov = b.solute_energy()
    assert not ov.any() and len(set(u_lj.tolist())) == R and len(set(u_real.tolist())) == R
    assert np.abs(u_lj).max() < 1e5, u_lj                          # no steric clash at the start


# ---- B1 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,n_groups", SHAPES)
def test_chains_in_every_row_stepped_by_the_oracle(shapes, replays, kernel, n_groups):
    got = shapes.big(kernel, n_groups)
    c = got["cand"]
    if kernel == 2:      # the wave kernel ran, on its candidate lists: its own counters hold every step once
        assert c["state"] == 1 and c["list_steps"] > 0 and c["list_steps"] + c["scan_steps"] == R * STEPS, c
    else:                # the workgroup-per-move kernel: no call prepared any list
        assert c["list_steps"] == 0 and c["scan_steps"] == 0 and c["bytes"] == 0 and c["state"] == 4, c
    assert np.abs(got["e1"] - got["fresh"]).max() < 1e-9 * np.abs(got["fresh"]).max(), (got["e1"], got["fresh"])
    worst = w_x = w_s = 0.0
    for r in PICKS:
        trace, e_acc, com_o, coords_o, S_o, tot_o = replays[r]
        at = (kernel, n_groups)
        worst = max(worst, check_trace(trace, got["d"], got["f"], r, at))
        com, coords, S = got["finals"][r]
        w_x = max(w_x, np.abs(com - com_o).max(), np.abs(coords - coords_o).max())
        w_s = max(w_s, np.abs(S - S_o).max())
        assert np.abs(com - com_o).max() < 2e-13 and np.abs(coords - coords_o).max() < 2e-13, (at, r)
        assert np.abs(S - S_o).max() < 1e-9, (at, r, np.abs(S - S_o).max())
        assert abs((got["e1"][r] - got["e0"][r]) - e_acc) < TOL * 1e5, (at, r)
        assert common.rel(got["fresh"][r], tot_o["energy"]) < TOL, (at, r, got["fresh"][r], tot_o["energy"])
    print(f"kernel {kernel} groups {n_groups}: replicas {PICKS}: largest |dU - oracle| {worst:.3e} K, "
          f"|x - oracle| {w_x:.3e} A (2e-13 allowed), |S(k) - oracle| {w_s:.3e} (1e-9 allowed); cand_stats {c}")


# ---- B2 ---------------------------------------------------------------------------------------------------
def same_bytes(big, shards):
    """[(replica, what)] that differ between the 37-replica batch and the shards."""
    bad = []
    for k, sh in zip(SHARDS, shards):
        for j in range(3):
            r = k + j
            pairs = [("dU", big["d"][r], sh["d"][j]), ("flags", big["f"][r], sh["f"][j]), ("e0", big["e0"][r], sh["e0"][j]),
                     ("e1", big["e1"][r], sh["e1"][j])]
            pairs += [(w, x, y) for w, x, y in zip(("com", "coords", "S(k)"), big["finals"][r], sh["finals"][j])]
            bad += [(r, w) for w, x, y in pairs if np.asarray(x).tobytes() != np.asarray(y).tobytes()]
    return bad


@pytest.mark.parametrize("kernel,n_groups", SHAPES)
def test_every_replica_is_the_small_shapes_bit_for_bit(shapes, kernel, n_groups):
    big, shards = shapes.big(kernel, n_groups), shapes.shards(kernel)
    assert sorted({k + j for k in SHARDS for j in range(3)}) == list(range(R)) and all(len(sh["finals"]) == 3 for sh in shards)
    bad = same_bytes(big, shards)
    n_acc = (big["f"] & 1).sum(1)
    print(f"kernel {kernel} groups {n_groups}: {len(bad)} differences from the shards of three; accepted steps per "
          f"replica {n_acc.min()} .. {n_acc.max()} of {STEPS}")
    assert not bad, bad[:12]
    assert n_acc.min() > 5 and len({big["d"][r].tobytes() for r in range(R)}) == R      # 37 chains of their own


def test_the_control_without_a_solute(shapes):
    """The same comparison on the path a solute forces, with no solute: a difference here is not the solute's."""
    bad = same_bytes(shapes.big(2, 2, solute=False), shapes.shards(2, solute=False))
    print(f"control without a solute, kernel 2, two groups: {len(bad)} differences from the shards of three")
    assert not bad, bad[:12]


# ---- B3 ---------------------------------------------------------------------------------------------------
OV_NEW, OV_OLD = (5, 22, 36), 20
BESIDE = (4, 6, 7, 21, 23)       # the rows that share a wave with an overlapping one


def rigid_to(com, at, d, box):
    """the molecule (com, at [3, 3]) moved rigidly by d, its centre of mass folded into the box"""
    d = (com + d) % box - com
    return com + d, at + d


@pytest.mark.parametrize("kernel", (1, 2))
def test_overlaps_stay_in_their_row(orc, water, kernel):
    a, box = water, float(water["box"])
    sol = sr.dipole(a)
    mol = sr.placed(sol.offsets, tsc.corner(box))       # upright: the negative site at c + (0.9, 0, 0)
    so = sr.SoluteOracle(orc, a, sol, LJ, QQ)
    reps = starts_around(a, mol, R, seed=38)
    rng = np.random.default_rng(5)
    touch = mol[1] + np.array([0.0, 0.5, 0.0])          # an H here is 0.5 A from the negative site
    picks, c_new, a_new = [], [], []
    for r in range(R):
        com, coords = reps[r]
        i = int(np.argmin(tsc.image_dist(com, mol[1], box)))
        at = coords[3 * i:3 * i + 3]
        if r == OV_OLD:      # starts in the overlap and proposes its way out
            com[i], coords[3 * i:3 * i + 3] = rigid_to(com[i], at, touch - at[1], box)
            cn, an = rigid_to(com[i], coords[3 * i:3 * i + 3], np.array([0.0, 3.0, 0.0]), box)
        elif r in OV_NEW:
            cn, an = rigid_to(com[i], at, touch - at[1], box)
        else:
            Rm = sr.rotation(rng) if r % 2 else np.eye(3)
            cn, an = rigid_to(com[i], com[i] + (at - com[i]) @ Rm.T, (rng.random(3) - 0.5) * 0.4, box)
        picks.append(i + 1)
        c_new.append(cn)
        a_new.append(an)
    want, ov_want = [], []
    for r in range(R):
        do, ovo = scr.N1(so, reps[r][0], reps[r][1], mol, box).trial(picks[r], c_new[r], a_new[r])
        want.append(do)
        ov_want.append(bool(ovo))
    assert [r for r in range(R) if ov_want[r]] == sorted(OV_NEW + (OV_OLD,)), ov_want
    with batch_with(a, reps, sol, mol, {"kernel": kernel}) as b:
        b.recip_long()
        if kernel == 2:
            b.set_parts(1)       # the wave kernel with one part per move: mmc_batch_eval prepares the candidate lists
        d, ov = b.eval(picks, c_new, a_new)
        b.settle(np.zeros(R, dtype=np.int32))
        c = b.cand_stats()
    if kernel == 2:
        assert c["state"] == 1 and c["list_steps"] + c["scan_steps"] == R, c
    leaked = [r for r in BESIDE if ov[r]]
    assert not leaked, f"replicas {leaked} of {BESIDE} report the overlap of the row beside them in their wave"
    assert [bool(x) for x in ov] == ov_want, (kernel, [r for r in range(R) if bool(ov[r]) != ov_want[r]])
    worst, bad = np.zeros(4), []
    for r in range(R):
        if ov_want[r]:
            continue
        for t, tn in enumerate(("d_lj", "d_real", "d_recip", "d_vir")):
            worst[t] = max(worst[t], abs(d[r, t] - want[r][t]))
            if not sr.solute_close(d[r, t], want[r][t], sol.n_sites):
                bad.append((r, tn, d[r, t], want[r][t]))
    print(f"kernel {kernel}: overlaps {[r for r in range(R) if ov[r]]}; largest |d_lj, d_real, d_recip, d_vir - oracle| of "
          f"the other {R - 4} replicas {worst} (1e-9 + 1e-13 |term| allowed); cand_stats {c}")
    assert not bad, bad[:8]


# ---- the observables beyond 1024 waters -------------------------------------------------------------------
N_BIG = 1090
GRIDS = ((12, 0.5), (3, 1.1))


class Big:
    """1090 SPC/E waters from the lattice, two replicas two device-proposed sweeps along; a place for a solute
    near the box's corner that keeps 2 A and more from every atom of both; and, per solute, replica 0 with
    waters planted by index (`planted`)."""

    def __init__(self):
        from test_gpu_npt import water_lattice
        self.a = a = water_lattice(N_BIG)
        self.box = box = float(a["box"])
        with make_batch(a, 2) as b:
            b.set_option("device_moves", 1)
            b.run(2 * N_BIG, T, 0.3, 0.2, seed=79)
            self.reps = [b.get_replica(r)[:2] for r in range(2)]
        rng = np.random.default_rng(11)
        atoms = np.vstack([c for _, c in self.reps])
        pts = (rng.random((4000, 3)) - 0.5) * 5.0      # within 2.5 A of the corner on every axis: the cube crosses faces
        dist = np.array([tsc.image_dist(atoms, p % box, box).min() for p in pts])
        self.c = pts[int(np.argmax(dist))] % box
        assert dist.max() > 2.0, dist.max()
        self._en = {}

    def solute(self, name):
        """(solute, mol): methane on the place; the dipole with its LJ site on it (the orientation the waters
        leave most room for)."""
        sol = tsc.solute_of(name, self.a)
        if name == "methane":
            return sol, sr.placed(sol.offsets, self.c)
        atoms = np.vstack([c for _, c in self.reps])
        best = None
        for seed in range(60):
            rot = sr.rotation(np.random.default_rng(seed))
            mol = sr.placed(sol.offsets, self.c - sol.offsets[0] @ rot.T, rot)
            room = min(tsc.image_dist(atoms, s, self.box).min() for s in mol[:-1])
            if best is None or room > best[0]:
                best = (room, mol)
        assert best[0] > 1.2, best[0]
        return sol, best[1]

    def planted(self, name):
        """(solute, mol, [(com, coords)] * 2): replica 0 with the waters 10 and 1034 (one thread of the map's
        1024) outside both cubes, 1050 without a frame, and against the dipole 1060 with an H 0.5 A from the
        negative site, against methane 1070 and 70 with their O 1.5 and 2.0 A from the site."""
        sol, mol = self.solute(name)
        box, c = self.box, mol[-1]
        com, coords = self.reps[0][0].copy(), self.reps[0][1].copy()

        def plant(i, target, anchor, atoms=None):
            at = coords[3 * i:3 * i + 3] if atoms is None else atoms
            cm = com[i] if atoms is None else atoms[0]
            d = np.asarray(target, dtype=float) - at[anchor]
            shift = -box * np.floor((cm + d) / box)
            com[i], coords[3 * i:3 * i + 3] = cm + d + shift, at + d + shift
        plant(10, c + [7.25, 1.0, 1.0], 0)
        plant(1034, c + [-1.0, -7.5, 2.0], 0)
        v = np.array([0.5, 0.25, 0.125])
        o = c + [-1.75, 1.75, -1.75]
        plant(1050, o, 0, atoms=np.array([o, o + v, o - v]))
        if name == "methane":
            plant(1070, mol[0] + [0.0, 0.0, 1.5], 0)
            plant(70, mol[0] + [0.0, -2.0, 0.0], 0)
        else:
            plant(1060, mol[1] + [0.0, 0.5, 0.0], 1)
        return sol, mol, [(com, coords), self.reps[1]]

    def energies(self, orc, name, sol, mol, reps):
        """The oracle's (u_lj, u_real, ov) [N] of BOTH replicas (2 x 1090 two-molecule calls take well under a second)."""
        if name not in self._en:
            so = sr.SoluteOracle(orc, self.a, sol, LJ, QQ)
            self._en[name] = [hm.water_energies(so, com, coords, mol, self.box) for com, coords in reps]
        return self._en[name]


@pytest.fixture(scope="module")
def big():
    return Big()


@pytest.mark.parametrize("name", ("dipole", "methane"))
def test_maps_rdf_and_energy_beyond_one_pass_of_the_stride(orc, big, name):
    sol, mol, reps = big.planted(name)
    a, box = big.a, big.box
    en = big.energies(orc, name, sol, mol, reps)
    fl = [hm.flagged(*e) for e in en]
    # what the planted waters are, on the oracle's values, before the device is asked
    assert not hm.bisector(reps[0][1], box)[1][1050] and hm.bisector(reps[0][1], box)[1].sum() == N_BIG - 1
    if name == "methane":
        u = en[0][0]
        print(f"methane: u_lj of water 1070 {u[1070]:.6g} K, of water 70 {u[70]:.6g} K; flagged {np.flatnonzero(fl[0])}")
        assert u[1070] > 2 * 2.0 ** 20 and fl[0][1070] and u[70] < 2.0 ** 19 and not fl[0][70]
        assert not en[0][2].any() and not en[1][2].any()            # no overlap flag anywhere: the solute is uncharged
    else:
        assert en[0][2][1060] and fl[0][1060] and en[0][2].sum() == 1 and not en[1][2].any()
    assert not fl[0][1050] and not fl[0][10] and not fl[0][1034] and not fl[1].any()
    so = sr.SoluteOracle(orc, a, sol, LJ, QQ)
    with tsc.batch_of(a, reps) as b:
        b.set_solute(sol, mol)
        b.recip_long()
        for n_half, cell in GRIDS:
            cells = (2 * n_half) ** 3
            sl = hm.slots(mol, reps[0][1], box, n_half, cell)
            assert sl[10, 0] == sl[1034, 0] == cells and sl[1050, 0] < cells
            for lo, hi in ((0, 1024), (1024, N_BIG)):   # both passes of the stride deposit inside and outside
                assert (sl[lo:hi, 0] < cells).any() and (sl[lo:hi, 0] == cells).any(), (n_half, cell, lo)
            want = np.array([hm.hydration_map(mol, coords, box, n_half, cell, *en[r]) for r, (_, coords) in enumerate(reps)])
            n_dep = np.array([hm.unflagged_counts(mol, coords, box, n_half, cell, fl[r]) for r, (_, coords) in enumerate(reps)])
            assert (want[0, 3:6, cells + 1] == 1).all() and want[0, 6, cells + 1] == want[0, 7, cells + 1] == fl[0].sum() >= 1
            for wgs in (0, 1):
                b.set_option("wave_wgs", wgs)
                per = b.hydration_map(n_half, cell, per_replica=True)
                tot = b.hydration_map(n_half, cell)
                assert per.shape == (2, 8, cells + 2) and tot.shape == (8, cells + 2)
                assert (per[:, :6] == want[:, :6]).all(), (name, n_half, cell, wgs)
                assert (tot[:6] == want[:, :6].sum(0)).all(), (name, n_half, cell, wgs)
                assert (per[:, :3].sum(2) == N_BIG).all()
                for r in range(2):
                    check_energy_rows(per[r, 6:], want[r, 6:], n_dep[r], f"{name} ({n_half}, {cell}) wave_wgs {wgs} replica {r}")
                check_energy_rows(tot[6:], want[:, 6:].sum(0), n_dep.sum(0), f"{name} ({n_half}, {cell}) wave_wgs {wgs} summed")
        b.set_option("wave_wgs", 0)
        # the radial histograms: 50 bins to 10 A
        ref = np.array([scr.rdf_solute_ref(mol, coords, box, 50, 10.0) for _, coords in reps])
        assert (b.rdf_solute(50, 10.0, per_replica=True) == ref).all() and (b.rdf_solute(50, 10.0) == ref.sum(0)).all()
        assert ref.sum() > 1000
        # the pair energy
        u_lj, u_real, u_ov = b.solute_energy()
        for r, (com, coords) in enumerate(reps):
            lj_o, real_o, ov_o = scr.N1(so, com, coords, mol, box).pair_energy()
            print(f"{name} replica {r}: u_lj {u_lj[r]!r} - oracle {u_lj[r] - lj_o:.3e}, u_real {u_real[r]!r} - oracle "
                  f"{u_real[r] - real_o:.3e}, overlap {bool(u_ov[r])}")
            assert bool(u_ov[r]) == ov_o == (name == "dipole" and r == 0)
            assert sr.solute_close(u_lj[r], lj_o, sol.n_sites) and sr.solute_close(u_real[r], real_o, sol.n_sites)


def test_a_chain_beside_the_wave_kernel_at_1090_waters(orc, big):
    """Kernel 2 with one part per move at 1090 waters: eighteen 64-molecule blocks to a full scan, the
    candidate lists in use, the solute's record beside every step; replica 1 replayed by the oracle."""
    a, box, steps, seed = big.a, big.box, 64, 1357
    sol, mol = big.solute("dipole")
    so = sr.SoluteOracle(orc, a, sol, LJ, QQ)
    got = run_chains(a, big.reps, sol, mol, {"device_moves": 1, "kernel": 2}, 2, steps=steps, seed=seed)
    c = got["cand"]
    assert c["state"] == 1 and c["list_steps"] > 0 and c["list_steps"] + c["scan_steps"] == 2 * steps, c
    n1 = scr.N1(so, big.reps[1][0], big.reps[1][1], mol, box)
    trace, e_acc, _ = scr.replay(n1, proposal_of(seed, 1, box), steps, T)
    worst = check_trace(trace, got["d"], got["f"], 1, "1090 waters")
    com, coords, S = got["finals"][1]
    n1.recip_long()
    w_x = max(np.abs(com - n1.s.com[:-1]).max(), np.abs(coords - n1.s.coords[:3 * N_BIG]).max())
    w_s = np.abs(S - n1.ew.sumQExpOld).max()
    n_acc = sum(f & 1 for _, f in trace)
    print(f"1090 waters, kernel 2: largest |dU - oracle| over {steps} steps {worst:.3e} K, |x - oracle| {w_x:.3e} A, "
          f"|S(k) - oracle| {w_s:.3e}; {n_acc} accepted; cand_stats {c}")
    assert w_x < 2e-13 and w_s < 1e-9
    assert abs((got["e1"][1] - got["e0"][1]) - e_acc) < TOL * 1e5
    assert np.abs(got["e1"] - got["fresh"]).max() < 1e-9 * np.abs(got["fresh"]).max()
    assert common.rel(got["fresh"][1], n1.potential()["energy"]) < TOL
    assert 0 < n_acc < steps
