"""Widom insertion (mmc_batch_widom / mmc_batch_widom_at) on every path it reads, against the oracle.

test_gpu_widom.py checks the terms on one shape: NIST configuration 4, one cutoff of 10 A, at most
64 insertions per replica, after the move server.  Here the rest of what k_widom_wave and
k_widom_reduce read or branch on:
  * the reduction past its first block of 64 insertions, with flagged insertions in later blocks,
    and the scratch buffers growing between calls;
  * separate LJ and Coulomb cutoffs (the prefilter takes the larger gate, the pair body its
    same_gate == false branch);
  * the neighbour list emptied mid-scan, so that the pair sums add across process() calls;
  * both sides of the molecule-image window (gate + r_mol_max + r_test against box / 2 and the
    slack), with caller-given and generated test molecules, after caller proposals and after
    quaternion chains;
  * the committed state (coordinates, S buffer, box, kappa) after every path that changes it;
  * TIP3P charges and the benchmark's own shape (61 440 replicas, 8 insertions each).
The oracle terms (common.widom_oracle_terms) recompute RecipLong from each replica's coordinates,
so a stale or wrong S(k) buffer shows in d_recip.  Tolerances as test_gpu_widom.py: 1e-9 K plus
1e-13 of each term, the overlap flag exact, the sums to 1e-14 of the host's in-order reduction."""
import math

import numpy as np
import pytest

import common
from common import check_widom, widom_host_sums

pytestmark = pytest.mark.gpu

T = 298.15
RC = 10.0


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def cfg4():
    return common.nist_arrays(4, "unwrapped")


def make_batch(a, R, lj=RC, qq=RC, recip=True):
    from metropolismontecarlo_amd import structs
    from metropolismontecarlo_amd.device import Batch
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
              5.6 / a["box"], structs.factor, lj, qq)
    if recip:
        b.recip_long()
    return b


def sums_close(bs, hb):
    """The library's sums against widom_host_sums: 1e-14 relative (equal where both overflowed)."""
    return np.all((bs == hb) | (np.abs(bs - hb) <= 1e-14 * np.abs(hb)))


def outputs_equal(x, y):
    return all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(x, y))


def rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def placed(off, com, rot=None):
    """A test molecule with body offsets `off` (3, 3), rotated by `rot`, at `com`: atoms (9), COM (3)."""
    o = np.asarray(off) if rot is None else np.asarray(off) @ rot.T
    return np.concatenate([(np.asarray(com) + o).ravel(), com])


def r_mol_max(a):
    d = np.asarray(a["coords"]) - np.repeat(np.asarray(a["com"]), 3, axis=0)
    return float(np.sqrt((d * d).sum(1)).max())


def img_bound(a, gate=RC, lj=RC, qq=RC):
    """The largest test-molecule extent for which mmc_widom.inc takes the molecule image:
    gate + r_mol_max + r_test + 1e-6 below box / 2 and below both slacks sqrt(r_cut^2 + 100)."""
    lim = min(0.5 * a["box"], math.sqrt(lj * lj + 100), math.sqrt(qq * qq + 100))
    return lim - gate - r_mol_max(a) - 1e-6


def stretched(off, r_test):
    """The offsets with atom 1 (an H) pushed out along its own direction to r_test from the COM."""
    o = np.array(off, dtype=float)
    o[1] *= r_test / np.linalg.norm(o[1])
    assert abs(np.linalg.norm(o, axis=1).max() - r_test) < 1e-12
    return o


# ---- 1. the reduction across blocks of 64 -------------------------------------------------------
@pytest.fixture(scope="module")
def three(cfg4):
    """NIST config 4, three replicas, each taken 100 device-proposed steps along its own chain."""
    b = make_batch(cfg4, 3)
    b.set_option("device_moves", 1)
    b.run(100, T, 0.3, 0.2, seed=515)
    yield b
    b.close()


def test_reduction_across_blocks(three):
    """M = 1 .. 200 (up to four blocks of k_widom_reduce) from non-zero starting sums: the host's
    in-order reduction of the returned dU, the same bytes for every launch shape."""
    b = three
    b0 = np.array([1e-3, 0.5, 7.25])
    n0 = np.array([3, 0, 11], dtype=np.int64)
    for M in (1, 63, 64, 65, 129, 200):
        runs = []
        for wgs in (0, 1, 2):
            b.set_option("wave_wgs", wgs)
            runs.append(b.widom(M, T, seed=1000 + M, draw0=3, boltz_sum=b0.copy(), n_overlap=n0.copy(),
                                outputs=True))
        b.set_option("wave_wgs", 0)
        bs, no, _, du, ovl = runs[0]
        hb, hn = widom_host_sums(du, ovl, b0, n0, T)
        assert np.array_equal(no, hn), (M, no, hn)
        assert sums_close(bs, hb), (M, bs, hb)
        assert np.all(bs >= b0) and (M == 1 or np.all(bs > b0)), M
        for other in runs[1:]:
            assert outputs_equal(runs[0], other), M


def test_flagged_insertions_in_later_blocks(three):
    """200 caller-given insertions per replica, overlaps and non-finite dU in the second and third
    blocks (and one in the first): flags, counts and sums against the host, for every launch shape."""
    b = three
    R, M = b.R, 200
    _, _, mol, _, _ = b.widom(M, T, seed=4711, outputs=True)
    off = b.widom_offsets
    plant = {}
    for r in range(R):
        com, coords, _ = b.get_replica(r)
        o = coords[3 * (100 + r)]
        over = placed(off, o + np.array([0.5, 0.0, 0.0]) - off[1])          # H 0.5 A from a foreign O
        dup = np.concatenate([coords[3 * (200 + r):3 * (200 + r) + 3].ravel(), com[200 + r]])   # a copy
        for j, m, f in ((5, over, 1), (70, over, 1), (100, dup, 2), (128, over, 1), (140, dup, 2),
                        (191, over, 1)):
            mol[r, j] = m
            plant[(r, j)] = f
    b0 = np.array([0.25, 0.0, 3.0])
    n0 = np.array([1, 2, 0], dtype=np.int64)
    runs = []
    for wgs in (0, 1, 2):
        b.set_option("wave_wgs", wgs)
        runs.append(b.widom_at(mol, T, boltz_sum=b0.copy(), n_overlap=n0.copy()))
    b.set_option("wave_wgs", 0)
    bs, no, du, ovl = runs[0]
    for (r, j), f in plant.items():
        assert ovl[r, j] == f, (r, j, ovl[r, j])
    assert np.count_nonzero(ovl) >= len(plant)
    hb, hn = widom_host_sums(du, ovl, b0, n0, T)
    assert np.array_equal(no, hn)
    assert sums_close(bs, hb), (bs, hb)
    for other in runs[1:]:
        assert outputs_equal(runs[0], other)


def test_scratch_growth_between_calls(cfg4):
    """M = 4, then 300 (the device and pinned scratch grow), then 4 again on one batch: each call
    bit for bit what the same call makes on a fresh batch."""
    calls = ((4, 21), (300, 22), (4, 23))
    with make_batch(cfg4, 3) as b:
        got = [b.widom(M, T, seed=s, boltz_sum=np.full(3, 0.5), outputs=True) for M, s in calls]
    for (M, s), g in zip(calls, got):
        with make_batch(cfg4, 3) as f:
            assert outputs_equal(g, f.widom(M, T, seed=s, boltz_sum=np.full(3, 0.5), outputs=True)), M


# ---- 2. separate cutoffs ------------------------------------------------------------------------
@pytest.mark.parametrize("lj,qq", [(8.0, 10.0), (10.0, 8.0)])
def test_separate_cutoffs(lj, qq, cfg4, orc):
    """LJ and Coulomb cutoffs apart: random insertions, and COMs at +-1e-12 relative of each gate
    around foreign COMs, against the oracle."""
    a = cfg4
    L = float(a["box"])
    with make_batch(a, 2, lj, qq) as b:
        b.set_option("device_moves", 1)
        b.run(60, T, 0.3, 0.2, seed=99)
        bs, no, mol, du, ovl = b.widom(24, T, seed=31, outputs=True)
        for r in range(2):
            check_widom(orc, a, b, r, mol[r], du[r], ovl[r], lj, qq, what=(lj, qq))
        off = b.widom_offsets
        dirs = (np.array([1.0, 0, 0]), np.array([0, 0, -1.0]), np.array([1.0, -1.0, 1.0]) / math.sqrt(3.0))
        mols = []
        for r in range(2):
            com, _, _ = b.get_replica(r)
            m = [placed(off, (com[j] + g * f * d) % L)
                 for j in (3, 250) for g in (lj, qq) for d in dirs for f in (1 - 1e-12, 1 + 1e-12)]
            mols.append(m)
        mols = np.array(mols)
        bs, no, du, ovl = b.widom_at(mols, T)
        for r in range(2):
            check_widom(orc, a, b, r, mols[r], du[r], ovl[r], lj, qq, what=(lj, qq, "gates"))


# ---- 3. the pair-list flush ---------------------------------------------------------------------
def test_neighbour_list_flush(orc):
    """2000 SPC/E molecules compressed to 0.06 / A^3 (32.2 A) with a 12.4 A cutoff: 430-520 COMs
    inside the gate of any point, so every scan of k_widom_wave empties its list after a trip and
    goes on (asserted on the host, common.scan_flushes): the pair sums add across process() calls.
    Test molecules at the centres of the lattice's cells, against the oracle."""
    from test_gpu_batch import _dense_water
    a = _dense_water(2000, rho=0.06)
    L, rc = float(a["box"]), 12.4
    assert rc < L / 2 and 5.6 / L * math.sqrt(rc * rc + 100) < 2.8
    nc = int(round(np.cbrt(2197)))
    sp = L / nc
    rng = np.random.default_rng(2000)
    cells = rng.choice(nc ** 3, size=24, replace=False)
    with make_batch(a, 1, rc, rc) as b:
        off = b.widom_offsets
        mols = []
        for c in cells:
            i, j, k = c // (nc * nc), (c // nc) % nc, c % nc
            com = (np.array([i, j, k]) + 0.51) * sp
            assert common.scan_flushes(a["com"], [com], rc, L), c
            mols.append(placed(off, com, rotation(rng)))
        mols = np.array(mols)[None]
        bs, no, du, ovl = b.widom_at(mols, T)
        check_widom(orc, a, b, 0, mols[0], du[0], ovl[0], rc, rc)


# ---- 4. the molecule-image window ---------------------------------------------------------------
def test_image_window_generated(cfg4, orc):
    """Generated insertions with stretched offsets: r_test just below the IMG bound (molecule image),
    just above it, and at 6.5 A, where the host finds atom pairs of gated molecule pairs whose
    image differs from their molecules' inside the slack.  Every case also with option
    image_by_molecule = 0 (the per-pair image): the same bytes."""
    a = cfg4
    bnd = img_bound(a)
    assert 3.17 < bnd < 3.18
    with make_batch(a, 2) as b:
        for r_test, seed in ((bnd - 1e-3, 5), (bnd + 1e-3, 6), (6.5, 7)):
            off = stretched(b.widom_offsets, r_test)
            out = b.widom(48, T, seed=seed, offsets=off, outputs=True)
            _, _, mol, du, ovl = out
            for r in range(2):
                check_widom(orc, a, b, r, mol[r], du[r], ovl[r], RC, RC, what=r_test)
            b.set_option("image_by_molecule", 0)
            assert outputs_equal(out, b.widom(48, T, seed=seed, offsets=off, outputs=True)), r_test
            b.set_option("image_by_molecule", -1)
            hits = []
            for r in range(2):
                com, coords, _ = b.get_replica(r)
                hits += [m for m in mol[r] if common.image_differs(m, com, coords, a["box"], RC, RC * RC + 100)]
            assert bool(hits) == (r_test == 6.5), (r_test, len(hits))


def test_image_window_caller_molecules(cfg4, orc):
    """widom_at, one set of stretched molecules per call (the extent is taken over the call's
    molecules): just below the bound and just above it, placed 10 (1 - 1e-9) A from a foreign COM
    with the stretched H pointing away from that molecule's farthest atom (just above the bound no
    atom pair can take another image yet: the host finds none); then r_test = 5.8 A along an axis,
    9.95 A from the foreign COM, where the H and the foreign atoms take another image than their
    molecules at r < 14 A.  Then COMs outside [0, L] by -1e-9 and by L 1e-15 (infinite extent: the
    per-pair image).  Each call also with image_by_molecule = 0: the same bytes."""
    a = cfg4
    L = float(a["box"])
    bnd = img_bound(a)
    com, coords = np.asarray(a["com"]), np.asarray(a["coords"])
    ext = coords - np.repeat(com, 3, axis=0)
    ext_n = np.linalg.norm(ext, axis=1).reshape(-1, 3)
    far_mols = np.argsort(-ext_n.max(1))[:6]

    def aim(u0, w):
        """The rotation taking the unit vector u0 onto the unit vector w (Rodrigues)."""
        ax = np.cross(u0, w)
        s, c = np.linalg.norm(ax), float(u0 @ w)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]]) / max(s, 1e-300)
        return np.eye(3) + s * K + (1 - c) * K @ K

    with make_batch(a, 1) as b:
        base = b.widom_offsets
        sets = []
        for r_test in (bnd - 1e-3, bnd + 1e-2):
            off = stretched(base, r_test)
            u0 = off[1] / np.linalg.norm(off[1])
            mols = []
            for j in far_mols:
                v = ext[3 * j + int(np.argmax(ext_n[j]))]
                v = v / np.linalg.norm(v)
                mols.append(placed(off, (com[j] - RC * (1 - 1e-9) * v) % L, aim(u0, -v)))
            sets.append((r_test, np.array(mols)[None]))
        off = stretched(base, 5.8)
        u0 = off[1] / np.linalg.norm(off[1])
        ex = np.array([1.0, 0.0, 0.0])
        lowest = np.argsort(ext[:, 0].reshape(-1, 3).min(1))[:6]        # an atom far out along -x
        sets.append((5.8, np.array([placed(off, (com[j] + 9.95 * ex) % L, aim(u0, ex)) for j in lowest])[None]))
        for r_test, mols in sets:
            out = b.widom_at(mols, T)
            check_widom(orc, a, b, 0, mols[0], out[2][0], out[3][0], RC, RC, what=r_test)
            hits = [m for m in mols[0] if common.image_differs(m, com, coords, L, RC, RC * RC + 100)]
            assert bool(hits) == (r_test == 5.8), (r_test, len(hits))
            b.set_option("image_by_molecule", 0)
            assert outputs_equal(out, b.widom_at(mols, T)), r_test
            b.set_option("image_by_molecule", -1)
        # COMs just outside the box
        mols = np.array([placed(base, np.array([-1e-9, 7.0, 12.0])),
                         placed(base, np.array([3.0, L * (1 + 1e-15), 20.0])),
                         placed(base, np.array([L * (1 + 1e-15), L * (1 + 1e-15), -1e-9]))])[None]
        assert mols[0, 1, 10] > L
        bs, no, du, ovl = b.widom_at(mols, T)
        check_widom(orc, a, b, 0, mols[0], du[0], ovl[0], RC, RC, what="outside")


def test_after_a_stretching_caller_proposal(cfg4, orc):
    """An accepted caller proposal (mmc_batch_eval + settle) leaves molecule 301 with an H 6.4 A from
    its COM: no bound on the molecules' extent any more (rigid_only false), so Widom must take the
    per-pair image.  Test molecules 9.9 A from that COM, on the far side from the H: the H and the
    test atoms are more than box / 2 apart along the axis, 13.7 A apart through the boundary.
    (mmc_batch.inc sets r_mol_max to infinity where it clears rigid_only, so each of the two keeps
    Widom's molecule image off on its own: this fails only if both are lost.)"""
    a = cfg4
    L = float(a["box"])
    i = 301
    with make_batch(a, 1) as b:
        com, coords, _ = b.get_replica(0)
        c = com[i - 1].copy()
        at = coords[3 * (i - 1):3 * i].copy()
        at[1] = c + np.array([6.4, 0.0, 0.0])
        b.eval(np.array([i]), c[None], at[None])
        b.settle(np.ones(1, dtype=np.int32))
        com, coords, _ = b.get_replica(0)
        assert np.array_equal(coords[3 * (i - 1) + 1], at[1])
        off = b.widom_offsets
        rng = np.random.default_rng(5)
        mols = np.array([placed(off, (c + np.array([-9.9, dy, dz])) % L, rotation(rng))
                         for dy in (-0.5, 0.0, 0.7) for dz in (-0.3, 0.4)])[None]
        hits = [m for m in mols[0] if i - 1 in common.image_differs(m, com, coords, L, RC, RC * RC + 100)]
        assert len(hits) == mols.shape[1]
        out = b.widom_at(mols, T)
        check_widom(orc, a, b, 0, mols[0], out[2][0], out[3][0], RC, RC)
        b.set_option("image_by_molecule", 0)
        assert outputs_equal(out, b.widom_at(mols, T))
        b.set_option("image_by_molecule", -1)
        bs, no, mol, du, ovl = b.widom(32, T, seed=12, outputs=True)
        check_widom(orc, a, b, 0, mol[0], du[0], ovl[0], RC, RC)


@pytest.mark.parametrize("mode", [1, 2])
def test_after_quaternion_chains(mode, orc):
    """200 steps of the quaternion route (mode 1 raises the molecules' bound past the image window
    of 216 molecules in 18.7 A at r_cut 7, mode 2 does not), then random insertions."""
    from test_gpu_replay_paths import Q_RCUT, system
    a, quat, db = system("q216", mode == 1)
    with make_batch(a, 2, Q_RCUT, Q_RCUT) as b:
        b.set_option("device_moves", 1)
        b.set_orientations(quat, db, faithful=mode == 1)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        b.run(200, T, 0.3, 0.3, seed=77, energies=e)
        bs, no, mol, du, ovl = b.widom(24, T, seed=8, outputs=True)
        for r in range(2):
            check_widom(orc, a, b, r, mol[r], du[r], ovl[r], Q_RCUT, Q_RCUT, what=mode)


# ---- 5. after every path that changes the committed state ---------------------------------------
def _widom_all(orc, a, b, M, seed, what):
    bs, no, mol, du, ovl = b.widom(M, T, seed=seed, outputs=True)
    for r in range(b.R):
        check_widom(orc, a, b, r, mol[r], du[r], ovl[r], RC, RC, what=what)
    hb, hn = widom_host_sums(du, ovl, np.zeros(b.R), np.zeros(b.R, dtype=np.int64), T)
    assert np.array_equal(no, hn) and sums_close(bs, hb)


def test_after_host_decided_runs(cfg4, orc):
    """One step per launch, the host decides (persistent = 0, accept_on_device = 0)."""
    with make_batch(cfg4, 8) as b:
        for k, v in (("device_moves", 1), ("kernel", 2), ("persistent", 0), ("accept_on_device", 0)):
            b.set_option(k, v)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        e, st = b.run(37, T, 0.3, 0.2, seed=5, energies=e)
        assert st["device_decisions"] == 0 and st["trans_accept"] + st["rot_accept"] > 0
        _widom_all(orc, cfg4, b, 12, 40, "host-decided")


@pytest.mark.parametrize("per_launch", [8, 16])
def test_after_kernel_decided_runs(per_launch, cfg4, orc):
    """Several steps per launch, the kernel decides, 24 replicas in two groups on one workgroup: the
    terms of every replica, and the chains go on bit for bit like a twin's that made no insertion."""
    R = 24
    opts = (("device_moves", 1), ("kernel", 2), ("persistent", 0), ("accept_on_device", 1),
            ("steps_per_launch", per_launch), ("wave_wgs", 1))
    with make_batch(cfg4, R) as b, make_batch(cfg4, R) as tw:
        es = []
        for x in (b, tw):
            for k, v in opts:
                x.set_option(k, v)
            e = x.potential_ewald(as_array=True)["energy"].copy()
            e, st = x.run(3 * per_launch + 5, T, 0.3, 0.2, seed=6, energies=e, n_groups=2, n_parts=1)
            assert st["device_decisions"] == R * (3 * per_launch + 5)
            es.append(e)
        _widom_all(orc, cfg4, b, 6, 41, per_launch)
        for x, k in ((b, 0), (tw, 1)):
            es[k], _ = x.run(2 * per_launch + 3, T, 0.3, 0.2, seed=7, energies=es[k], n_groups=2, n_parts=1)
        assert es[0].tobytes() == es[1].tobytes()
        for r in range(R):
            assert outputs_equal(b.get_replica(r), tw.get_replica(r)), r


def test_after_the_latency_server(cfg4, orc):
    """One replica with the default options: the latency server runs the chain."""
    with make_batch(cfg4, 1) as b:
        b.set_option("device_moves", 1)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        e, st = b.run(150, T, 0.3, 0.2, seed=8, energies=e, n_groups=1)
        assert st["server_steps"] == 150
        _widom_all(orc, cfg4, b, 32, 42, "latency")


def test_after_eval_and_settle(cfg4, orc):
    """Caller proposals with the host's decisions, one of them accepted: the committed S(k) is in
    the other buffer (s_cur = 1) for every replica."""
    a = cfg4
    R = 2
    com, coords = np.asarray(a["com"]), np.asarray(a["coords"])
    with make_batch(a, R) as b:
        d = np.array([0.2, -0.1, 0.15])
        b.eval(np.full(R, 5), np.tile(com[4] + d, (R, 1)), np.tile(coords[12:15] + d, (R, 1, 1)))
        b.eval(np.full(R, 9), np.tile(com[8] - d, (R, 1)), np.tile(coords[24:27] - d, (R, 1, 1)),
               accept_prev=np.ones(R, dtype=bool))
        b.settle(np.zeros(R, dtype=np.int32))
        c1, x1, _ = b.get_replica(1)
        assert np.array_equal(c1[4], com[4] + d) and np.array_equal(c1[8], com[8])
        _widom_all(orc, a, b, 16, 43, "eval/settle")


def test_volume_trial_accept_and_reject(cfg4, orc):
    """One replica: between mmc_batch_volume_trial and its decision Widom is refused and writes
    nothing; after a reject the same call gives the same bytes as before the trial; after an
    accept the terms in the new box (get_boxes, kappa = 5.6 / box)."""
    from metropolismontecarlo_amd import _lib
    a = cfg4
    L1 = (1.01 * a["box"] ** 3) ** (1 / 3)
    with make_batch(a, 1) as b:
        b.set_option("device_moves", 1)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        b.run(80, T, 0.3, 0.2, seed=9, energies=e, n_groups=1)
        before = b.widom(40, T, seed=44, outputs=True)
        for accept in (False, True):
            b.volume_trial(L1, 5.6 / L1)
            bs, no = np.full(1, 7.5), np.full(1, 3, dtype=np.int64)
            with pytest.raises(_lib.MMCError) as ei:
                b.widom(4, T, 1, boltz_sum=bs, n_overlap=no)
            assert ei.value.status == _lib.MMC_ERR_STATE and bs[0] == 7.5 and no[0] == 3
            with pytest.raises(_lib.MMCError) as ei:
                b.widom_at(np.full((1, 1, 12), 5.0), T, boltz_sum=bs, n_overlap=no)
            assert ei.value.status == _lib.MMC_ERR_STATE and bs[0] == 7.5 and no[0] == 3
            if accept:
                b.volume_accept()
            else:
                b.volume_reject()
                assert outputs_equal(before, b.widom(40, T, seed=44, outputs=True))
        assert b.get_boxes()[0] == L1
        _widom_all(orc, a, b, 24, 45, "volume accept")


def test_after_run_npt(cfg4, orc):
    """mmc_batch_run_npt on one replica: the terms at the final box of get_boxes()."""
    a = cfg4
    with make_batch(a, 1) as b:
        b.set_option("device_moves", 1)
        e0 = float(b.potential_ewald(as_array=True)["energy"][0])
        e1, st, ns = b.run_npt(8, T, 0.03, 0.05 * a["box"] ** 3, 0.3, 0.2, 13, e0, moves_per_sweep=40)
        assert ns["vol_attempt"] == 8
        _widom_all(orc, a, b, 24, 46, ("npt", float(b.get_boxes()[0]), ns["vol_accept"]))


def test_after_set_replica_and_recip_long(cfg4, orc):
    """mmc_batch_set_replica on one replica of three, then mmc_batch_recip_long."""
    a = cfg4
    L = float(a["box"])
    com, coords = np.asarray(a["com"]), np.asarray(a["coords"])
    with make_batch(a, 3) as b:
        shift = np.array([1.3, -2.1, 0.4])
        c2 = (com + shift) % L
        x2 = coords + np.repeat(c2 - com, 3, axis=0)
        c2[10] += np.array([0.3, 0.2, -0.1])
        x2[30:33] += np.array([0.3, 0.2, -0.1])
        b.set_replica(1, c2, x2)
        b.recip_long()
        assert np.array_equal(b.get_replica(1)[0], c2)
        _widom_all(orc, a, b, 16, 47, "set_replica")


# ---- 6. TIP3P -----------------------------------------------------------------------------------
def test_tip3p_lattice(orc):
    from test_gpu_npt import water_lattice
    a = water_lattice(1000, "tip3p")
    with make_batch(a, 2) as b:
        b.set_option("device_moves", 1)
        b.run(100, T, 0.3, 0.2, seed=10)
        _widom_all(orc, a, b, 24, 48, "tip3p")


# ---- 7. the benchmark's shape -------------------------------------------------------------------
def test_bench_shape(cfg4, orc):
    """61 440 replicas of NIST config 4, 8 insertions each, after a two-group run in which the kernel
    decides: replicas at the edges of k_widom_wave's unit -> wave map (unit r M + j, at most
    4 WIDOM_OCC / WV_WAVES workgroups per compute unit) against the oracle, and every replica's sum
    against the host's reduction of the returned dU."""
    R, M = 61440, 8
    check = common.replicas_by_wave_position(R, 1, n_cus=common.device_cu_count(), parts=M,
                                             occ=common.widom_occ())
    assert len(check) >= 4
    with make_batch(cfg4, R, recip=False) as b:
        for k, v in (("device_moves", 1), ("kernel", 2), ("accept_on_device", 1)):
            b.set_option(k, v)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        e, st = b.run(16, T, 0.316555789, 0.05, seed=11, energies=e, n_groups=2, n_parts=1)
        assert st["device_decisions"] == 16 * R
        b0 = np.full(R, 0.125)
        bs, no, mol, du, ovl = b.widom(M, T, seed=49, draw0=16, boltz_sum=b0.copy(), outputs=True)
        for r, where in check.items():
            check_widom(orc, cfg4, b, r, mol[r], du[r], ovl[r], RC, RC, what=where)
        hb, hn = widom_host_sums(du, ovl, b0, np.zeros(R, dtype=np.int64), T)
        assert np.array_equal(no, hn)
        assert sums_close(bs, hb)
