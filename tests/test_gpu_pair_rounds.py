"""k_move_eval_wave decides once per round (64 neighbours) and state whether an atom pair came closer
than sqrt(ovr): the nine atom pairs run with the gate as their only mask, and only a round that
trips the test is run again through the exact body (overlap sentinel of ewalds.jl:359, the series
below r^2 = 0.25).  These tests put such a pair where the fallback has to act -- first round, second
round, old state, new state, both, lanes 0 / 63 / 64+, a wave that goes on to other units, a scan
that empties its list -- and replay every dU, overlap flag and decision through the oracle:

  * scripted moves (mmc_batch_eval: one step per launch, the host decides), every step's four dU
    terms and overlap flag against orc.trial_move, the final state byte for byte;
  * the driver with device proposals from a state that holds the close pair: eight steps per launch
    with the kernel deciding (final state, sum of accepted dU, accept and overlap counts), and one
    step per launch with the host deciding (every step's dU and flags, option "trace_steps").

The COM gate is r_cut itself (mmc_pair_params, diameter 0), the scan's 16-bit prefilter admits at
most ~2e-3 A more: list positions are computed here from COM distances, away from that margin.
Tolerance: TOL = 1e-9 of the per-molecule energy scale, as tests/test_gpu_batch.py and the series
test of tests/test_gpu_perbox_paths.py."""
import math

import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu

TOL = 1e-9
T, DR, DPHI = 298.15, 0.316555789, 0.05
OVR = 0.5          # r^2 below which opposite charges overlap (ewalds.jl:359)
R_OV = 0.5         # an H placed this far from an O: r^2 = 0.25 < ovr
R_COLD = 0.42      # an H placed this far from an H: r^2 < MMC_QQ_UMIN = 0.25, the table's end


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def make_batch(a, R, rcut):
    from metropolismontecarlo_amd import structs
    from metropolismontecarlo_amd.device import Batch
    return Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
                 5.6 / a["box"], structs.factor, rcut, rcut)


def _mi(d, L):
    return d - L * np.round(d / L)


# ---- geometry: where a close pair sits in the scan's list ------------------------------------------
def list_position(com, centres, j, rcut, box, margin):
    """(lowest, highest) position molecule j can have in the neighbour list of a unit whose old and
    new centres are `centres`: the molecules before j (the moved one included: the scan lets it
    through) whose COM is within r_cut of a centre, those within `margin` of the gate counted
    both ways."""
    d = np.min([np.linalg.norm(_mi(com[:j] - np.asarray(c), box), axis=1) for c in centres], axis=0)
    return int(np.sum(d < rcut - margin)), int(np.sum(d < rcut + margin))


def rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def place(a, m, j, site_m, site_j, dist, n_try=4000):
    """Molecule m (0-based) turned and shifted rigidly so that its atom site_m lies `dist` from atom
    site_j of molecule j, every other opposite-charge pair it makes at 1.2 A or more and every
    other like-charge pair at 0.9 A or more: ONE close pair.  Returns (com_new, atoms_new)."""
    L, X, q = a["box"], a["coords"], a["charge"]
    body = X[3 * m:3 * m + 3] - a["com"][m]
    others = np.ones(X.shape[0], dtype=bool)
    others[3 * m:3 * m + 3] = False
    rng = np.random.default_rng(1000 * m + j)
    opp = q[3 * m:3 * m + 3][:, None] * q[others][None, :] < 0
    target = np.zeros_like(opp)
    target[site_m, int(np.sum(others[:3 * j + site_j]))] = True
    for _ in range(n_try):
        Rm = rotation(rng)
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        nb = body @ Rm.T
        com_new = X[3 * j + site_j] + dist * u - nb[site_m]
        atoms = com_new + nb
        d = np.linalg.norm(_mi(atoms[:, None, :] - X[None, others, :], L), axis=2)
        if d[opp & ~target].min() >= 1.2 and d[~opp & ~target].min() >= 0.9:
            return com_new, atoms
    raise AssertionError(("no placement", m, j))


def close_pair(a, m, rcut, want, like=False, margin=0.7, j_range=None, held=True):
    """(j, com_new, atoms_new): molecule m placed on a neighbour j -- an H of m R_OV from j's O, or
    with like=True R_COLD from an H of j -- such that j's position lies in want = (lo, hi) in the
    list of the move that takes m there (scanned from both COMs) and, with held=True, in the list of
    a small move from there as well."""
    for j in (j_range if j_range is not None else range(a["com"].shape[0])):
        if j == m:
            continue
        com_new, atoms = place(a, m, j, 1, 1 if like else 0, R_COLD if like else R_OV)
        com = a["com"].copy()
        com[m] = com_new
        lo, hi = list_position(com, [com_new, a["com"][m]], j, rcut, a["box"], margin)
        if held:
            lo2, hi2 = list_position(com, [com_new], j, rcut, a["box"], margin)
            lo, hi = min(lo, lo2), max(hi, hi2)
        if want[0] <= lo and hi < want[1]:
            return j, com_new, atoms
    raise AssertionError(("no neighbour at positions", want))


def with_molecule(a, m, com_new, atoms):
    com, X = a["com"].copy(), a["coords"].copy()
    com[m] = com_new
    X[3 * m:3 * m + 3] = atoms
    return dict(a, com=com, coords=X)


def closest(a, opposite):
    """Smallest distance between atoms of different molecules with opposite / like charges."""
    L, X, q = a["box"], a["coords"], a["charge"]
    mol = np.repeat(np.arange(X.shape[0] // 3), 3)
    best = np.inf
    for i in range(0, X.shape[0], 300):
        d = np.linalg.norm(_mi(X[i:i + 300, None, :] - X[None, :, :], L), axis=2)
        sel = (mol[i:i + 300, None] != mol[None, :]) & ((q[i:i + 300, None] * q[None, :] < 0) == opposite)
        best = min(best, d[sel].min())
    return best


# ---- the two replays ---------------------------------------------------------------------------------
def scripted(orc, states, rcut, moves, rules, wave_wgs=0):
    """moves[n][r] = (mol 0-based, com_new, atoms_new) through mmc_batch_eval, replica r from
    states[r] with accept rule rules[r](n): every step's dU terms and overlap flag against the
    oracle, the final state byte for byte.  Returns the overlap flags [n][r]."""
    R = len(states)
    s = [common.oracle_system(a) for a in states]
    ew = [orc.Ewald(5.6 / a["box"], 5, 27, a["box"]) for a in states]
    flags = []
    with make_batch(states[0], R, rcut) as b:
        b.set_option("kernel", 2)
        if wave_wgs:
            b.set_option("wave_wgs", wave_wgs)
        for r, a in enumerate(states):
            b.set_replica(r, a["com"], a["coords"])
            orc.recip_long(ew[r], s[r].coords, s[r].charge, a["box"])
        b.recip_long()
        acc_prev = np.zeros(R, dtype=bool)
        for n, mv in enumerate(moves):
            d, ov = b.eval(np.array([x[0] + 1 for x in mv]), np.array([x[1] for x in mv]),
                           np.array([x[2] for x in mv]), acc_prev)
            row = []
            for r in range(R):
                i, cn, an = mv[r]
                do, ovo = orc.trial_move(i + 1, s[r], ew[r], rcut, rcut, cn, an)
                print(f"step {n} replica {r}: overlap {ovo}, |dU - oracle| {np.abs(d[r] - do).max():.3e}")
                assert bool(ov[r]) == bool(ovo), (n, r)
                assert np.abs(d[r] - do).max() < TOL * (np.abs(do).max() + 1e4), (n, r, d[r], do)
                acc = bool(rules[r](n)) and not ovo
                if acc:
                    s[r].com[i] = cn
                    s[r].coords[3 * i:3 * i + 3] = an
                    ew[r].sumQExpOld = ew[r].sumQExpNew.copy()
                else:
                    ew[r].sumQExpNew = ew[r].sumQExpOld.copy()
                acc_prev[r] = acc
                row.append(bool(ovo))
            flags.append(row)
        b.settle(acc_prev)
        for r in range(R):
            com, coords, S = b.get_replica(r)
            assert np.array_equal(com, s[r].com) and np.array_equal(coords, s[r].coords), r
            assert np.abs(S - ew[r].sumQExpOld).max() < 1e-11 * np.abs(ew[r].sumQExpOld).max(), r
    return flags


def oracle_replay(orc, a, replica, n_steps, seed, rcut):
    """tests/test_gpu_batch.py's oracle_replay for one call at any cutoff."""
    from test_gpu_batch import _rigid_proposal
    s = common.oracle_system(a)
    box, n_mol = a["box"], a["com"].shape[0]
    ew = orc.Ewald(5.6 / box, 5, 27, box)
    orc.recip_long(ew, s.coords, s.charge, box)
    e_acc, n_acc, n_ovl, trace = 0.0, 0, 0, []
    for step in range(n_steps):
        i = step % n_mol
        kind, c_new, a_new, u = _rigid_proposal(seed, replica, step, s.com[i].copy(),
                                                s.coords[3 * i:3 * i + 3].copy(), box, DR, DPHI)
        d, ov = orc.trial_move(i + 1, s, ew, rcut, rcut, c_new, a_new)
        delta = d[0] + d[1] + d[2]
        x = delta / T
        accept = (x < 0.0 or math.exp(-x) > u) and not ov
        trace.append((delta, int(accept) | (int(ov) << 1) | (kind << 2)))
        n_ovl += bool(ov)
        if accept:
            e_acc += delta
            n_acc += 1
            s.com[i] = c_new
            s.coords[3 * i:3 * i + 3] = a_new
            ew.sumQExpOld = ew.sumQExpNew.copy()
        else:
            ew.sumQExpNew = ew.sumQExpOld.copy()
    return dict(com=s.com, coords=s.coords, S=ew.sumQExpOld, e_acc=e_acc, n_acc=n_acc, n_ovl=n_ovl, trace=trace)


def driven(orc, states, rcut, n_steps, seed=4711, wave_wgs=0, replica0=2):
    """The driver with device proposals from states[r], twice: eight steps per launch with the
    kernel deciding, and one step per launch with the host deciding and every step traced.  The
    oracle steps the same chains.  Returns the oracle's replays."""
    R = len(states)
    replays = [oracle_replay(orc, a, replica0 + r, n_steps, seed, rcut) for r, a in enumerate(states)]
    for on_device in (1, 0):
        with make_batch(states[0], R, rcut) as b:
            b.set_option("kernel", 2)
            b.set_option("device_moves", 1)
            b.set_option("persistent", 0)
            b.set_option("accept_on_device", on_device)
            if on_device:
                b.set_option("steps_per_launch", 8)
            else:
                b.set_option("trace_steps", n_steps)
            if wave_wgs:
                b.set_option("wave_wgs", wave_wgs)
            for r, a in enumerate(states):
                b.set_replica(r, a["com"], a["coords"])
            e0 = b.potential_ewald(as_array=True)["energy"].copy()
            e1, st = b.run(n_steps, T, DR, DPHI, seed=seed, energies=e0, n_groups=min(R, 2), n_parts=1,
                           n_threads=2, replica0=replica0)
            if on_device:
                assert st["device_decisions"] == R * n_steps and st["launches"] == min(R, 2) * -(-n_steps // 8), st
            else:
                assert st["device_decisions"] == 0
                d_gpu, f_gpu = b.get_trace(n_steps)
            final = [b.get_replica(r) for r in range(R)]
        print(f"kernel decides {on_device}: overlaps {st['overlaps']}, oracle {sum(o['n_ovl'] for o in replays)}")
        assert st["overlaps"] == sum(o["n_ovl"] for o in replays), st
        assert st["trans_accept"] + st["rot_accept"] == sum(o["n_acc"] for o in replays), st
        for r, o in enumerate(replays):
            if not on_device:
                for step, (delta, flags) in enumerate(o["trace"]):
                    assert abs(d_gpu[r, step] - delta) < TOL * (abs(delta) + 1e4), (r, step, d_gpu[r, step], delta)
                    assert f_gpu[r, step] == flags, (r, step)
            com, coords, S = final[r]
            assert np.abs(com - o["com"]).max() < 2e-13 and np.abs(coords - o["coords"]).max() < 2e-13, r
            assert np.abs(S - o["S"]).max() < 1e-11 * np.abs(o["S"]).max(), r
            assert abs((e1[r] - e0[r]) - o["e_acc"]) < TOL * (abs(o["e_acc"]) + 1e5), r
    return replays


def shifted(a, i, d):
    return (i, a["com"][i] + d, a["coords"][3 * i:3 * i + 3] + d)


RULES = [lambda n: True, lambda n: False, lambda n: n % 2 == 0]
M = 3   # the molecule that is placed on a neighbour: step 3 of the driver's first launch moves it


def fallback_in_a_round(orc, cfg, rcut, want, like, one_round=False):
    """(a), (b), (c): the close pair at list positions `want` of a NIST configuration.  Scripted:
    from the clean state a move INTO the close pair (new state only); from the state that holds it
    a small move (both states), the move back out (old state only), a move of a molecule elsewhere,
    and a move of the neighbour itself (old state, the pair at another position of another list).
    Then the driver from the state that holds it."""
    a = common.nist_arrays(cfg, "unwrapped")
    # (one round: a neighbour near the molecule's own place, so that the move there lists little more)
    near = np.argsort(np.linalg.norm(_mi(a["com"] - a["com"][M], a["box"]), axis=1)) if one_round else None
    j, com_p, atoms_p = close_pair(a, M, rcut, want, like, j_range=near)
    held = with_molecule(a, M, com_p, atoms_p)
    if one_round:   # everything the placed molecule's scans can list, from either centre
        assert list_position(held["com"], [com_p, a["com"][M]], a["com"].shape[0], rcut, a["box"], 0.1)[1] < 64
    if like:   # no overlap anywhere, one like-charge pair below the table's end
        assert closest(held, True) > 1.0 and closest(held, False) < 0.45
    else:
        assert closest(a, True) > 1.0 and closest(held, True) < math.sqrt(OVR)
    far = next(k for k in range(a["com"].shape[0])
               if np.linalg.norm(_mi(a["com"][k] - com_p, a["box"])) > 6.0 and k not in (M, j))
    tiny, small = np.array([0.004, -0.003, 0.002]), np.array([0.05, 0.04, -0.03])
    into = [[(M, com_p, atoms_p)] * 3, [shifted(a, M, small)] * 3, [(M, com_p, atoms_p)] * 3, [shifted(a, far, small)] * 3]
    f = scripted(orc, [a] * 3, rcut, into, RULES)
    if not like:
        assert f == [[True] * 3, [False] * 3, [True] * 3, [False] * 3], f
    out = [[shifted(held, M, tiny)] * 3, [(M, a["com"][M], a["coords"][3 * M:3 * M + 3])] * 3,
           [shifted(held, far, small)] * 3, [shifted(held, j, tiny)] * 3, [shifted(held, M, -tiny)] * 3]
    f = scripted(orc, [held] * 3, rcut, out, RULES)
    if like:
        assert not np.any(f), f
    else:   # every move that touches the pair is an overlap and is rejected: the pair stays
        assert f == [[True] * 3, [True] * 3, [False] * 3, [True] * 3, [True] * 3], f
    replays = driven(orc, [held] * 6, rcut, 16)
    if not like:   # step M moves the placed molecule: an overlap in every chain, and rejected
        assert all(o["trace"][M][1] & 2 for o in replays) and all(o["n_ovl"] >= 1 for o in replays)
        assert all(np.array_equal(o["com"][M], com_p) for o in replays)


@pytest.mark.parametrize("want", [(0, 60), (64, 124)], ids=["first-round", "second-round"])
def test_overlap_fallback_two_round_list(want, orc):
    """(a) 200 molecules (NIST configuration 2; ~104 of them inside a 10 A gate: two rounds), an H
    0.5 A from a neighbour's O, the neighbour in the first round of the list, then in the second."""
    fallback_in_a_round(orc, 2, 10.0, want, like=False)


@pytest.mark.parametrize("want", [(0, 60), (64, 124)], ids=["first-round", "second-round"])
def test_series_below_the_table_two_round_list(want, orc):
    """(b) the same with two H of different molecules 0.42 A apart and no opposite charges close:
    no overlap, the exact body takes the series for that pair and dU is the oracle's."""
    fallback_in_a_round(orc, 2, 10.0, want, like=True)


def test_overlap_fallback_single_round_list(orc):
    """(c) 100 molecules (NIST configuration 1) at r_cut = 8 A, ~27 inside the gate: the list is one
    round also for the move that brings the molecule to its neighbour, scanned from both places
    (at 10 A that move lists ~80)."""
    fallback_in_a_round(orc, 1, 8.0, (0, 64), like=False, one_round=True)


def test_overlap_fallback_after_the_list_was_emptied(orc):
    """(d) NIST configuration 4 at r_cut = 12.4 A, about the largest cutoff the table kernels take
    (r_cut^2 + 100 must stay inside the table's 256 A^2: r_cut <= 12.49; 14 A, ~320 neighbours, is
    refused): ~220 molecules inside the gate, four rounds, the close pair with a
    neighbour beyond the first trip of the scan (molecule 400 on), and a replica without one.  Its
    first trip (384 molecules) leaves ~115 in the list, fewer than the WV_LIST - 64 WV_PF = 256
    that make the scan empty it (common.scan_flushes says so below).  The list IS emptied mid-scan
    in the second system: 2000 molecules compressed to 0.06 / A^3 at r_cut = 12.4 A, where every
    scan does, with the close pair in the list made after that, and a replica without one."""
    a = common.nist_arrays(4, "unwrapped")
    rcut = 12.4
    j, com_p, atoms_p = close_pair(a, M, rcut, (100, 400), j_range=range(400, 750))
    assert not common.scan_flushes(a["com"], [a["com"][M], com_p], rcut, a["box"], exclude=M)
    small = np.array([0.05, 0.04, -0.03])
    f = scripted(orc, [a] * 3, rcut, [[(M, com_p, atoms_p)] * 3, [shifted(a, M, small)] * 3, [shifted(a, 700, small)] * 3], RULES)
    assert f == [[True] * 3, [False] * 3, [False] * 3], f
    driven(orc, [with_molecule(a, M, com_p, atoms_p), a], rcut, 8)

    from test_gpu_batch import _dense_water
    a = _dense_water(2000, rho=0.06)
    rcut = 12.4
    j, com_p, atoms_p = close_pair(a, M, rcut, (300, 640), j_range=range(1500, 2000))
    assert common.scan_flushes(a["com"], [a["com"][M], com_p], rcut, a["box"], exclude=M)
    assert common.scan_flushes(a["com"], [a["com"][M]], rcut, a["box"], exclude=M)
    f = scripted(orc, [a] * 2, rcut, [[(M, com_p, atoms_p)] * 2, [shifted(a, M, small)] * 2, [shifted(a, 1990, small)] * 2],
                 RULES[:2])
    assert f == [[True] * 2, [False] * 2, [False] * 2], f
    driven(orc, [with_molecule(a, M, com_p, atoms_p), a], rcut, 8)


def test_fallback_lane_and_the_units_after_it(orc):
    """(e) NIST configuration 4 at the bench's cutoff (the minimum image by molecule, the bench's
    instantiation), one workgroup per launch: each wave runs three replicas in a row.  The lane that
    trips the fallback is lane 0, lane 63 and a lane of the second round (list positions 0, 63 and
    64+ of the move that makes the pair, exact: no COM within 0.004 A of the gate before the
    neighbour; the driver's chains then start from the state that holds it); every fourth replica has no
    close pair.  A replica with one is followed on its wave by one with another kind or none, so
    sums restored for one unit that leaked into the next would show there."""
    a = common.nist_arrays(4, "unwrapped")
    rcut, R = 10.0, 12
    kinds = {}
    for name, want in (("lane 0", (0, 1)), ("lane 63", (63, 64)), ("second round", (70, 120))):
        kinds[name] = close_pair(a, M, rcut, want, margin=0.004, held=False)
    order = ["lane 0", "lane 63", "second round", None]
    kind = [order[(r + r // 4) % 4] for r in range(R)]
    assert all(len({kind[w], kind[w + 4], kind[w + 8]}) == 3 for w in range(4))
    placed = [(M, kinds[k][1], kinds[k][2]) if k else shifted(a, M, np.array([0.03, 0.02, -0.04])) for k in kind]
    small = np.array([0.05, 0.04, -0.03])
    rules = [(lambda n: True) if r % 2 else (lambda n: False) for r in range(R)]
    f = scripted(orc, [a] * R, rcut, [placed, [shifted(a, M + 1, small)] * R, placed, [shifted(a, 400, -small)] * R],
                 rules, wave_wgs=1)
    want = [k is not None for k in kind]
    assert f == [want, [False] * R, want, [False] * R], f
    states = [with_molecule(a, M, kinds[k][1], kinds[k][2]) if k else a for k in kind]
    replays = driven(orc, states, rcut, 8, wave_wgs=1)
    assert [o["n_ovl"] >= 1 for o in replays] == want
