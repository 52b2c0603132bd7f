"""Per-replica boxes on the paths they branch on (mmc_batch_set_boxes, include/mmc_hip.h), each
against the oracle or against a one-box batch that must agree bit for bit:

- totals and RecipLong at the batch sizes that pick a different kernel path: the paired per-box
  totals ((n_mol + 1) / 2 * R >= 4096), RecipLong chunked (R <= 15), in one chunk (16 <= R <= 248)
  and a wave per column (R >= 249), R = 1 (four S(k) buffers per replica), and an odd molecule
  count above 768;
- every replica's erfc table (mmc_batch_qq_table_replica) against a one-box table and mpmath,
  also after a mixed batched volume move;
- trial-move chains against one-box chains, per part count and stream layout;
- the erfc series below r^2 = 0.25, the only place the fast kernels read a replica's own kappa
  and not its table;
- chains at other shapes replayed by the oracle, overlaps, repeated set_boxes.

Helpers and tolerances are those of test_gpu_npt_replicas.py."""
import functools

import numpy as np
import pytest

import common
from common import rel
from test_gpu_npt_replicas import ALPHA, DPHI, DR, RCUT, T, TOL, host_rescale, oracle_npt_chain

pytestmark = pytest.mark.gpu
KEYS = ("energy", "virial", "lj", "real", "recip", "self")


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


# ---- helpers -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nist(k):
    return common.nist_arrays(k, "unwrapped")


@functools.lru_cache(maxsize=None)
def lattice(n_mol):
    from test_gpu_npt import water_lattice
    return water_lattice(n_mol, "spce")


def at_boxes(a, boxes):
    return [host_rescale(a, float(L)) for L in boxes]


def make_batch(states, lj=RCUT, qq=RCUT):
    """A batch built from states[0] whose replica r holds states[r] in its own box; S(k) built."""
    from metropolismontecarlo_amd import structs
    from metropolismontecarlo_amd.device import Batch
    a0 = states[0]
    b = Batch(len(states), a0["com"], a0["coords"], a0["atype"], a0["charge"], a0["eps"], a0["sig"],
              a0["box"], ALPHA / a0["box"], structs.factor, lj, qq)
    for r, a in enumerate(states):
        b.set_replica(r, a["com"], a["coords"])
    b.set_boxes([a["box"] for a in states], ALPHA)
    b.recip_long()
    return b


def one_box_batch(a, lj=RCUT, qq=RCUT, R=1):
    """R copies of one state in one box: the trial-move kernel and proposals per-box mode uses
    (kernel 1, device-side proposals, no move server)."""
    from metropolismontecarlo_amd import structs
    from metropolismontecarlo_amd.device import Batch
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
              ALPHA / a["box"], structs.factor, lj, qq)
    b.set_option("kernel", 1)
    b.set_option("persistent", 0)
    b.set_option("device_moves", 1)
    b.recip_long()
    return b


def oracle_totals(orc, a, lj=RCUT, qq=RCUT):
    L = a["box"]
    return orc.potential_ewald(common.oracle_system(a), orc.Ewald(ALPHA / L, 5, 27, L), lj, qq)


def spread_boxes(R, lo=24.0, hi=36.0):
    """R distinct boxes in [lo, hi], in a fixed shuffled order (the extremes are not the ends)."""
    if R == 1:
        return np.array([27.3])
    return np.random.default_rng(R).permutation(np.linspace(lo, hi, R))


def checked_replicas(boxes, n_spread=4):
    """First, last, smallest box, largest box, and a few spread through the range."""
    R = len(boxes)
    idx = {0, R - 1, int(np.argmin(boxes)), int(np.argmax(boxes))}
    idx |= {int(i) for i in np.linspace(0, R - 1, n_spread + 2)[1:-1]}
    return sorted(idx)


def same_replica(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x, y))


def assert_totals(t, r, to, what):
    for key in KEYS:
        assert rel(t[key][r], to[key], 1.0) < TOL, (what, r, key, t[key][r], to[key])
    assert t["n_overlap"][r] == 0 and to["n_overlap"] == 0, (what, r)


# ---- 1. totals and RecipLong across the R-dependent paths ----------------------------------------
def check_totals_and_reversal(orc, states, what):
    """The checked replicas against the oracle; all replicas bit for bit against a batch holding
    the same states in reversed order (its replica R - 1 - r is replica r)."""
    boxes = np.array([a["box"] for a in states])
    with make_batch(states) as b, make_batch(states[::-1]) as rb:
        t = b.potential_ewald(as_array=True).copy()
        e = b.recip_long()
        for r in checked_replicas(boxes):
            to = oracle_totals(orc, states[r])
            assert_totals(t, r, to, (what, boxes[r]))
            assert rel(e[r] * b.factor, to["recip"]) < TOL, (what, r)
        tr = rb.potential_ewald(as_array=True)
        er = rb.recip_long()
        for key in KEYS + ("n_overlap",):
            assert np.array_equal(tr[key][::-1], t[key]), (what, key)
        assert np.array_equal(er[::-1], e), what


@pytest.mark.parametrize("R", [1, 12, 16, 256])
def test_totals_and_recip_long_at_every_batch_size_path(R, orc):
    """NIST configuration 4 at R distinct boxes in [24, 36]: R = 1 (four S(k) buffers), R = 12
    (paired totals: 375 * 12 >= 4096; RecipLong in chunks), R = 16 (RecipLong in one chunk),
    R = 256 (RecipLong with a wave per column)."""
    check_totals_and_reversal(orc, at_boxes(nist(4), spread_boxes(R)), f"NIST 4, R = {R}")


@pytest.mark.parametrize("R", [3, 12])
def test_totals_with_an_odd_molecule_count_above_768(R, orc):
    """801 SPC/E molecules (more than MMC_PRE COM-scan blocks, 401 molecule pairs per replica):
    R = 3 runs the one-molecule units, R = 12 the paired ones (401 * 12 >= 4096)."""
    a = lattice(801)
    check_totals_and_reversal(orc, at_boxes(a, spread_boxes(R, 0.92 * a["box"], 1.08 * a["box"])),
                              f"801 molecules, R = {R}")


# ---- 2. the table of every replica ---------------------------------------------------------------
TABLE_BOXES = (20.0, 20.5, 22.0, 25.0, 27.5, 30.0, 33.0, 36.0)   # L = 2 r_cut ... 36


def table_points(kappa, n=1200, seed=3):
    rng = np.random.default_rng(seed)
    u_hi = min(255.999, 16.0 / kappa ** 2)    # kappa * r <= 4
    u = np.concatenate([
        np.exp(rng.uniform(np.log(0.25), np.log(u_hi), n)),       # the table proper
        np.exp(rng.uniform(np.log(1e-4), np.log(0.25), n // 8)),  # the series below r^2 = 0.25
        [0.25, np.nextafter(0.25, 0), 0.5, 1.0, u_hi],
        2.0 ** np.arange(-2, 8) * (1 + 1.0 / 16),                 # piece boundaries
    ])
    return u[u <= u_hi]


def test_every_replica_holds_the_table_of_its_own_kappa():
    """kappa = alpha / L from L = 2 r_cut (kappa * sqrt(r_cut^2 + 100) = 3.96) to 36: each
    replica's table equals a one-box batch's at that kappa bit for bit, and stays within
    test_gpu_table.py's bounds against mpmath."""
    from metropolismontecarlo_amd._lib import MMCError
    from test_gpu_table import exact
    states = at_boxes(nist(1), TABLE_BOXES)
    with make_batch(states) as b:
        for r, a in enumerate(states):
            kappa = ALPHA / a["box"]
            u = table_points(kappa)
            got = b.qq_table(u, replica=r)
            with one_box_batch(a) as b1:
                assert np.array_equal(got, b1.qq_table(u)), r
                assert np.array_equal(got, b1.qq_table(u, replica=0)), r   # one box: the shared table
            ref = exact(kappa, u)
            err = np.abs(got - ref) / ref
            assert err.max() < 4e-14, (a["box"], u[err.argmax()], err.max())
            near = kappa * np.sqrt(u) <= 2.5
            assert err[near].max() < 5e-15, (a["box"], u[near][err[near].argmax()], err[near].max())
        for bad in (lambda: b.qq_table([1.0], replica=-1), lambda: b.qq_table([1.0], replica=len(states)),
                    lambda: b.qq_table([0.0], replica=0), lambda: b.qq_table([256.0], replica=0)):
            with pytest.raises(MMCError, match="MMC_ERR_ARG"):
                bad()
        assert b.qq_table([], replica=1).shape == (0,)


def test_tables_follow_a_mixed_volume_settle():
    """During a batched volume trial a moved replica holds the table of alpha / L_new and every
    other replica's table is untouched; after a mixed settle accepted replicas keep the new table,
    rejected and unmoved ones hold their old one bit for bit."""
    boxes = np.array([21.0, 24.0, 27.0, 30.0, 33.0, 36.0])
    new = np.array([22.5, 0.0, 25.0, 29.0, 0.0, 34.0])
    accept = np.array([1, 1, 0, 1, 0, 0], dtype=np.int32)
    states = at_boxes(nist(1), boxes)
    u = table_points(ALPHA / 20.0, n=300)

    def one_box_table(L):
        with one_box_batch(host_rescale(nist(1), L)) as b1:
            return b1.qq_table(u)

    with make_batch(states) as b:
        before = [b.qq_table(u, replica=r) for r in range(len(boxes))]
        b.volume_trial_replicas(new)
        for r in range(len(boxes)):
            want = one_box_table(new[r]) if new[r] else before[r]
            assert np.array_equal(b.qq_table(u, replica=r), want), ("trial", r)
        b.volume_settle(accept)
        assert np.array_equal(b.get_boxes(), np.where((new != 0) & (accept != 0), new, boxes))
        for r in range(len(boxes)):
            want = one_box_table(new[r]) if new[r] and accept[r] else before[r]
            assert np.array_equal(b.qq_table(u, replica=r), want), ("settled", r)


# ---- 3. trial-move chains against one-box chains -------------------------------------------------
S_ONE_LAUNCH = 2e-14   # |S(k)| difference of k_potential_one's and the phase kernels' sums (1.2e-14 seen)


@pytest.mark.parametrize("n_parts", [1, 4])
def test_trial_move_chains_equal_one_box_chains(n_parts):
    """Replica r of a per-box batch against one-box batches at box_r drawing from the same stream
    (replica0 = r): the same kernel arithmetic (the library builds with -ffp-contract=off), so
    running energies, centres of mass, atoms and accept counts agree bit for bit.  S(k) too,
    against a two-replica one-box batch.  A one-replica one-box batch builds its first S(k) in one
    launch (k_potential_one, DeviceSystem::recip_long_all), a different summation order from the
    phase kernels every per-box batch uses: its S(k) differs by a few ulps, by as much at the end
    as at the start, and nothing the chain decides or adds up moves."""
    states = at_boxes(nist(4), (27.0, 30.0, 33.5))
    steps, seed = 60, 9191
    with make_batch(states) as b:
        e0 = b.potential_ewald(as_array=True)["energy"].copy()
        s_start = [b.get_replica(r)[2] for r in range(len(states))]
        e1, st = b.run(steps, T, DR, DPHI, seed=seed, energies=e0.copy(), n_parts=n_parts)
        reps = [b.get_replica(r) for r in range(len(states))]
    acc = np.zeros(2, dtype=np.int64)
    for r, a in enumerate(states):
        with one_box_batch(a) as b1, one_box_batch(a, R=2) as b2:
            d_start = np.abs(b1.get_replica(0)[2] - s_start[r]).max()
            e, st1 = b1.run(steps, T, DR, DPHI, seed=seed, energies=e0[r:r + 1].copy(),
                            n_parts=n_parts, replica0=r)
            e2, _ = b2.run(steps, T, DR, DPHI, seed=seed, energies=np.repeat(e0[r], 2),
                           n_parts=n_parts, replica0=r)
            assert e[0] == e1[r] and e2[0] == e1[r], (r, e[0] - e1[r], e2[0] - e1[r])
            com, coords, sk = b1.get_replica(0)
            assert np.array_equal(com, reps[r][0]) and np.array_equal(coords, reps[r][1]), r
            d_end = np.abs(sk - reps[r][2]).max()
            assert d_start < S_ONE_LAUNCH and d_end < S_ONE_LAUNCH, (r, d_start, d_end)
            assert same_replica(b2.get_replica(0), reps[r]), r
        acc += (st1["trans_accept"], st1["rot_accept"])
    assert tuple(acc) == (st["trans_accept"], st["rot_accept"])
    assert 0 < acc.sum() < steps * len(states)


# ---- 4. stream layout ----------------------------------------------------------------------------
def test_stream_layout_does_not_change_per_box_chains():
    """Energies, statistics, coordinates and S(k) are identical bit for bit whatever the number of
    replica groups and worker threads, over two calls in a row."""
    states = at_boxes(nist(4), spread_boxes(7, 26.0, 34.0))
    res = []
    for groups, threads in ((1, 1), (3, 2), (2, 2)):
        with make_batch(states) as b:
            e = b.potential_ewald(as_array=True)["energy"].copy()
            stats = []
            for n in (23, 17):
                e, st = b.run(n, T, DR, DPHI, seed=515, energies=e, n_groups=groups, n_threads=threads)
                stats.append([st[q] for q in ("moves", "trans_accept", "rot_accept", "overlaps")])
            res.append((e.copy(), stats, [b.get_replica(r) for r in range(len(states))]))
    for other in res[1:]:
        assert np.array_equal(res[0][0], other[0]) and res[0][1] == other[1]
        assert all(same_replica(x, y) for x, y in zip(res[0][2], other[2]))
    assert res[0][1][0][0] == 23 * len(states)


# ---- 5. the erfc series with each replica's kappa ------------------------------------------------
SERIES_BOXES = (25.0, 27.0, 30.0, 32.0)
HH = 0.42   # the H-H distance built in (the series covers r < 0.5)


def _rotation(qv):
    w, x, y, z = qv / np.linalg.norm(qv)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _min_image(d, L):
    return d - L * np.round(d / L)


@functools.lru_cache(maxsize=None)
def close_pair_placement(n_try=3000, seed=5):
    """A rigid placement of molecule 1 of NIST configuration 4 with one of its H atoms HH from an H
    of molecule 0: the rotation, direction and H pair that keep opposite charges and the other
    molecules farthest away (seeded search)."""
    a = nist(4)
    L, X, q = a["box"], a["coords"], a["charge"]
    body = X[3:6] - a["com"][1]
    near = np.r_[np.arange(0, 3), np.arange(6, X.shape[0])]
    near = near[np.linalg.norm(_min_image(X[near] - X[1], L), axis=1) < 8.0]
    opp = q[3:6][:, None] * q[near][None, :] < 0
    third = np.broadcast_to(near[None, :] >= 6, opp.shape)
    rng = np.random.default_rng(seed)
    best = None
    for t in range(n_try):
        Rm = _rotation(rng.normal(size=4))
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        h0, h1 = 1 + t % 2, 1 + (t // 2) % 2
        atoms = body @ Rm.T
        d = np.linalg.norm(_min_image((X[h0] + HH * u - atoms[h1] + atoms)[:, None, :] - X[None, near, :], L),
                           axis=2)
        score = min(d[opp].min() - 1.2, d[third].min() - 2.4)
        if best is None or score > best[0]:
            best = (score, atoms, u, h0, h1)
    return best[1:]


def close_pair_state(L):
    """NIST configuration 4 rescaled to L, then molecule 1 placed by close_pair_placement."""
    atoms, u, h0, h1 = close_pair_placement()
    a = host_rescale(nist(4), L)
    com, X = a["com"].copy(), a["coords"].copy()
    c = X[h0] + HH * u - atoms[h1]
    com[1] = c % L
    X[3:6] = com[1] + atoms
    return dict(a, com=com, coords=X)


def check_close_pair(orc, a):
    """One like-charge pair (H-H) below 0.5 A, every opposite-charge pair at 1 A or more (the
    trial move's overlap radius), no overlap for the oracle."""
    L, X, q = a["box"], a["coords"], a["charge"]
    d = np.linalg.norm(_min_image(X[:, None, :] - X[None, :, :], L), axis=2)
    same = np.repeat(np.arange(X.shape[0] // 3), 3)
    inter = same[:, None] != same[None, :]
    like = inter & (q[:, None] * q[None, :] > 0)
    assert 0.3 <= d[like].min() <= 0.45 and np.sum(d[like] < 0.5) == 2, d[like].min()
    assert d[inter & (q[:, None] * q[None, :] < 0)].min() > 1.0
    to = oracle_totals(orc, a)
    assert to["n_overlap"] == 0
    return to


SERIES_CHAIN = dict(seed=2718, n_sweeps=3, per_sweep=12, vmax_frac=0.01, pressure=0.0)


def test_series_below_half_an_angstrom_uses_each_replicas_kappa(orc):
    """The state with an H-H pair at 0.42 A at four boxes: totals against the oracle, then a chain
    whose sweeps move molecules 0 and 1 (each sweep starts at molecule 0), replayed by the oracle.
    The batch's kappa in place of the replica's would shift each such pair by ~10^3 K."""
    states = [close_pair_state(L) for L in SERIES_BOXES]
    with make_batch(states) as b:
        t = b.potential_ewald(as_array=True).copy()
        for r, a in enumerate(states):
            assert_totals(t, r, check_close_pair(orc, a), "close pair")
        c = SERIES_CHAIN
        vmax = c["vmax_frac"] * states[0]["box"] ** 3
        e1, st, ns = b.run_npt_replicas(c["n_sweeps"], T, c["pressure"], vmax, DR, DPHI, c["seed"],
                                        t["energy"].copy(), moves_per_sweep=c["per_sweep"], alpha=ALPHA)
        check_chains(orc, b, states, e1, st, ns, c["seed"], [c["pressure"]] * len(states), vmax,
                     c["n_sweeps"], c["per_sweep"])


# ---- 6. chains at other shapes, replayed by the oracle -------------------------------------------
def check_chains(orc, b, states, e1, st, ns, seed, pressures, vmax, n_sweeps, per_sweep, lj=RCUT,
                 qq=RCUT, replica0=0):
    """Every replica of `b` after run_npt_replicas against oracle_npt_chain; returns the oracle's
    volume-move log of every replica."""
    logs, n_acc = [], 0
    boxes = b.get_boxes()
    t_end = b.potential_ewald(as_array=True)
    for r, a in enumerate(states):
        log = []
        box, com, coords, energy, acc, acc_vol = oracle_npt_chain(
            orc, a, replica0 + r, pressures[r], vmax, seed, n_sweeps, per_sweep, rc=qq, lj_rc=lj, log=log)
        assert ns[r]["vol_attempt"] == n_sweeps and ns[r]["vol_accept"] == acc_vol, (r, log)
        assert ns[r]["box"] == pytest.approx(box, rel=1e-15) and boxes[r] == ns[r]["box"], r
        gcom, gcoords, _ = b.get_replica(r)
        assert np.abs(gcom - com).max() < 1e-11 and np.abs(gcoords - coords).max() < 1e-11, r
        assert abs(e1[r] - energy) < TOL * abs(energy), (r, e1[r] - energy)
        assert rel(t_end["energy"][r], energy) < TOL, r
        n_acc += acc
        logs.append(log)
    assert st["trans_accept"] + st["rot_accept"] == n_acc
    flat = sum(logs, [])
    assert "accepted" in flat and "rejected" in flat, "parameters must accept some volume moves and reject some"
    return logs


def test_chains_at_twice_the_cutoff_refuse_small_boxes(orc):
    """NIST configuration 1 (100 molecules) from L = 20 = 2 r_cut and just above it, with a vmax
    that proposes boxes below 2 r_cut: those are refused outright, others accepted or rejected."""
    states = at_boxes(nist(1), (20.0, 20.01, 20.05, 20.2))
    seed, n_sweeps, per_sweep, vmax = 31337, 6, 50, 120.0
    pressures = (0.0, 0.05, 0.1, 0.2)
    with make_batch(states) as b:
        e0 = b.potential_ewald(as_array=True)["energy"].copy()
        e1, st, ns = b.run_npt_replicas(n_sweeps, T, 0.0, vmax, DR, DPHI, seed, e0,
                                        moves_per_sweep=per_sweep, alpha=ALPHA, pressures=pressures)
        logs = check_chains(orc, b, states, e1, st, ns, seed, pressures, vmax, n_sweeps, per_sweep)
    assert "refused" in sum(logs, [])
    assert min(ns[r]["box"] for r in range(len(states))) >= 2 * RCUT


def test_chains_with_different_lj_and_coulomb_cutoffs(orc):
    """NIST configuration 4 with lj_rcut = 8 and qq_rcut = 10: the fast kernel's separate gates."""
    states = at_boxes(nist(4), (28.5, 30.0, 31.5))
    seed, n_sweeps, per_sweep, vmax = 1618, 4, 30, 0.02 * 30.0 ** 3
    pressures = (0.0, 0.05, 0.1)
    with make_batch(states, lj=8.0, qq=10.0) as b:
        t = b.potential_ewald(as_array=True).copy()
        for r, a in enumerate(states):
            assert_totals(t, r, oracle_totals(orc, a, lj=8.0, qq=10.0), "lj 8")
        e1, st, ns = b.run_npt_replicas(n_sweeps, T, 0.0, vmax, DR, DPHI, seed, t["energy"].copy(),
                                        moves_per_sweep=per_sweep, alpha=ALPHA, pressures=pressures)
        check_chains(orc, b, states, e1, st, ns, seed, pressures, vmax, n_sweeps, per_sweep, lj=8.0, qq=10.0)


def test_chains_above_768_molecules(orc):
    """801 SPC/E molecules at two boxes: several LDS tiles per move."""
    a = lattice(801)
    states = at_boxes(a, (a["box"], 1.03 * a["box"]))
    seed, n_sweeps, per_sweep, vmax = 4242, 4, 40, 0.02 * a["box"] ** 3
    pressures = (0.0, 0.05)
    with make_batch(states) as b:
        e0 = b.potential_ewald(as_array=True)["energy"].copy()
        e1, st, ns = b.run_npt_replicas(n_sweeps, T, 0.0, vmax, DR, DPHI, seed, e0,
                                        moves_per_sweep=per_sweep, alpha=ALPHA, pressures=pressures)
        check_chains(orc, b, states, e1, st, ns, seed, pressures, vmax, n_sweeps, per_sweep)


def test_two_npt_calls_in_a_row_continue_the_chain(orc):
    """run_npt_replicas twice (2 then 3 sweeps) equals one oracle replay of 5 sweeps: the volume
    draws continue the Philox step count, and every sweep restarts the molecule order."""
    states = at_boxes(nist(4), (29.0, 30.5))
    seed, per_sweep, vmax, rep0 = 8080, 25, 0.02 * 30.0 ** 3, 5
    pressures = (0.0, 0.1)
    with make_batch(states) as b:
        e = b.potential_ewald(as_array=True)["energy"].copy()
        tot = dict(trans_accept=0, rot_accept=0)
        vol = np.zeros(len(states), dtype=np.int64)
        for n_sweeps in (2, 3):
            e, st, ns = b.run_npt_replicas(n_sweeps, T, 0.0, vmax, DR, DPHI, seed, e,
                                           moves_per_sweep=per_sweep, alpha=ALPHA, pressures=pressures,
                                           replica0=rep0)
            for k in tot:
                tot[k] += st[k]
            vol += [x["vol_accept"] for x in ns]
        for r in range(len(states)):
            ns[r]["vol_attempt"], ns[r]["vol_accept"] = 5, int(vol[r])
        check_chains(orc, b, states, e, tot, ns, seed, pressures, vmax, 5, per_sweep, replica0=rep0)


# ---- 7. overlaps ---------------------------------------------------------------------------------
L_OVERLAP = 20.0   # NIST configuration 4 rescaled to L = 20 has overlapping atom pairs


def test_an_overlapping_replica_reports_infinity_and_leaves_the_others_alone(orc):
    boxes = (26.0, L_OVERLAP, 30.0, 34.0)
    states = at_boxes(nist(4), boxes)
    assert oracle_totals(orc, states[1])["n_overlap"] > 0
    with make_batch(states) as b:
        t = b.potential_ewald(as_array=True)
        assert t["energy"][1] == np.inf and t["n_overlap"][1] == 1   # as include/mmc_hip.h says
        for r in (0, 2, 3):
            assert_totals(t, r, oracle_totals(orc, states[r]), "next to an overlap")


def test_a_rejected_move_into_an_overlapping_box_restores_the_replica(orc):
    states = at_boxes(nist(4), (24.0, 27.0, 30.0))
    assert oracle_totals(orc, host_rescale(states[0], L_OVERLAP))["n_overlap"] > 0
    with make_batch(states) as b, make_batch(states) as twin:
        t0 = b.potential_ewald(as_array=True).copy()
        before = [b.get_replica(r) for r in range(3)]
        tot = b.volume_trial_replicas([L_OVERLAP, 0.0, 0.0])
        assert tot["energy"][0] == np.inf and tot["n_overlap"][0] == 1
        b.volume_settle([0, 0, 0])
        assert np.array_equal(b.get_boxes(), [24.0, 27.0, 30.0])
        assert all(same_replica(before[r], b.get_replica(r)) for r in range(3))
        t1 = b.potential_ewald(as_array=True).copy()
        assert all(np.array_equal(t1[k], t0[k]) for k in KEYS)
        t2 = twin.potential_ewald(as_array=True)
        e1, st1 = b.run(40, T, DR, DPHI, seed=61, energies=t1["energy"].copy())
        e2, st2 = twin.run(40, T, DR, DPHI, seed=61, energies=t2["energy"].copy())
        assert np.array_equal(e1, e2) and st1["trans_accept"] == st2["trans_accept"]
        assert all(same_replica(b.get_replica(r), twin.get_replica(r)) for r in range(3))


# ---- 8. repeated set_boxes and one replica -------------------------------------------------------
def test_set_boxes_twice_equals_a_batch_built_at_the_second_boxes():
    states = at_boxes(nist(4), (26.0, 29.0, 33.0))
    with make_batch(states) as direct:
        want = direct.potential_ewald(as_array=True).copy()
        want_recip = direct.recip_long()
    with make_batch(states) as b:
        b.set_boxes([31.0, 25.0, 35.0], ALPHA)
        b.recip_long()
        b.set_boxes([a["box"] for a in states], ALPHA)
        assert np.array_equal(b.recip_long(), want_recip)
        t = b.potential_ewald(as_array=True)
        assert all(np.array_equal(t[k], want[k]) for k in KEYS)


def test_one_replica_per_box_batch_against_one_box_npt():
    """R = 1: run_npt_replicas against the one-box run_npt of make_one_replica_batch (different
    totals kernels: to 1e-12, like test_npt_replicas_equal_one_replica_batches)."""
    from test_gpu_npt import make_one_replica_batch
    a = host_rescale(nist(4), 29.0)
    seed, n_sweeps, per_sweep, vmax, P = 777, 4, 30, 0.02 * 29.0 ** 3, 0.05
    with make_batch([a]) as b:
        e0 = b.potential_ewald(as_array=True)["energy"].copy()
        e1, st, ns = b.run_npt_replicas(n_sweeps, T, P, vmax, DR, DPHI, seed, e0,
                                        moves_per_sweep=per_sweep, alpha=ALPHA, replica0=2)
    with make_one_replica_batch(a) as b1:
        f0 = float(b1.potential_ewald(as_array=True)["energy"][0])
        assert rel(f0, e0[0]) < 1e-12
        f1, st1, ns1 = b1.run_npt(n_sweeps, T, P, vmax, DR, DPHI, seed, f0, moves_per_sweep=per_sweep,
                                  alpha=ALPHA, replica0=2)
    assert ns1["vol_accept"] == ns[0]["vol_accept"] and ns1["vol_attempt"] == ns[0]["vol_attempt"]
    assert ns1["box"] == ns[0]["box"]
    assert rel(f1, e1[0]) < 1e-12
    assert st1["trans_accept"] + st1["rot_accept"] == st["trans_accept"] + st["rot_accept"]


def test_one_replica_volume_settle_restores_everything():
    """R = 1 keeps four S(k) buffers per replica: a rejected volume move gives them all back (the
    chain afterwards equals a twin's), an accepted one leaves the rescaled state."""
    a = host_rescale(nist(4), 28.0)
    with make_batch([a]) as b, make_batch([a]) as twin:
        e = b.potential_ewald(as_array=True)["energy"].copy()
        e, _ = b.run(30, T, DR, DPHI, seed=12, energies=e)
        f = twin.potential_ewald(as_array=True)["energy"].copy()
        f, _ = twin.run(30, T, DR, DPHI, seed=12, energies=f)
        before = b.get_replica(0)
        b.volume_trial_replicas([28.5])
        b.volume_settle([0])
        assert same_replica(before, b.get_replica(0)) and b.get_boxes()[0] == 28.0
        e, _ = b.run(30, T, DR, DPHI, seed=13, energies=e)
        f, _ = twin.run(30, T, DR, DPHI, seed=13, energies=f)
        assert np.array_equal(e, f) and same_replica(b.get_replica(0), twin.get_replica(0))
        before = b.get_replica(0)
        b.volume_trial_replicas([28.5])
        b.volume_settle([1])
        com, coords, _ = b.get_replica(0)
        want = host_rescale(dict(a, com=before[0], coords=before[1]), 28.5)
        assert b.get_boxes()[0] == 28.5
        assert np.array_equal(com, want["com"]) and np.array_equal(coords, want["coords"])
