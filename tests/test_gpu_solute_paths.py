"""Widom insertion of foreign solutes and of solute pairs (mmc_batch_widom_solute / _at,
mmc_batch_widom_pair / _at) on every path they read, against the oracle.

test_gpu_solute.py and test_gpu_solute_pair.py check the terms on one shape: NIST configuration 4, one
cutoff of 10 A, 2 to 5 separations, at most 65 insertions, after a device-proposed run().  Here the
rest of what k_solute_wave, k_solute_pair_wave and k_pair_reduce read or branch on:
  1. separate LJ and Coulomb cutoffs: the prefilter on the larger gate, the gates g and l per water
     and for the A-B term, on either side of each;
  2. the site counts at the edges: charged solutes of 4 and 5 sites (k_solute_wave<4> / <16>), pairs
     of (15, 1), (1, 15) and (8, 8) sites, a pair with exactly one uncharged solute;
  3. 1, 7 and 32 separations (one short tile, two full tiles, nine tiles), 0 and 33 refused;
  4. systems of 1 .. 257 molecules (the scans' clamp and their trips of 256);
  5. the committed state (coordinates, S buffer, box, kappa) after every path that changes it;
  6. flagged insertions of every kind in the later blocks of k_pair_reduce;
  7. the generated B placements against their host mirror, the Philox counter across 2^32;
  8. the shared observable scratch between calls of different layouts.
Every term against solute_ref.SoluteOracle / solute_pair_ref.PairOracle with solute_ref.solute_close
(1e-9 max(1, S / 3) K plus 1e-13 of the term), the overlap bits exact, the sums to 1e-14 of the
host's in-order reduction, placements to 1e-12 A of the mirror, and the same bytes where the library
promises them.  The oracle recomputes RecipLong(N) for every placement (cache=False): a kept value
would hide a stale S buffer.  tests/test_solute_paths_host.py holds the preconditions."""
import numpy as np
import pytest

import common
import solute_pair_ref as pr
import solute_ref as sr
from metropolismontecarlo_amd import _lib
from metropolismontecarlo_amd import observables as obs
from metropolismontecarlo_amd import structs

pytestmark = pytest.mark.gpu

T, RC, SUMS = sr.T, pr.RCUT, pr.SUMS


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def cfg4():
    return common.nist_arrays(4, "unwrapped")


def make_batch(a, R, lj=RC, qq=RC, alpha=5.6):
    from metropolismontecarlo_amd.device import Batch
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
              alpha / a["box"], structs.factor, lj, qq)
    b.recip_long()
    return b


@pytest.fixture(scope="module")
def two(cfg4):
    """NIST config 4, two replicas, each taken 60 device-proposed steps along its own chain."""
    b = make_batch(cfg4, 2)
    b.set_option("device_moves", 1)
    b.run(60, T, 0.3, 0.2, seed=98)
    yield b
    b.close()


@pytest.fixture(scope="module")
def three(cfg4):
    """NIST config 4, three replicas, each taken 100 device-proposed steps along its own chain."""
    b = make_batch(cfg4, 3)
    b.set_option("device_moves", 1)
    b.run(100, T, 0.3, 0.2, seed=515)
    yield b
    b.close()


def flat(out):
    """The arrays of a call's outputs, in a fixed order."""
    if isinstance(out, dict):
        return [np.asarray(out[k]) for k in sorted(out)]
    if isinstance(out, (tuple, list)):
        return [x for o in out for x in flat(o)]
    return [np.asarray(out)]


def same(x, y):
    fx, fy = flat(x), flat(y)
    return len(fx) == len(fy) and all(u.tobytes() == v.tobytes() for u, v in zip(fx, fy))


def within_twice(x, y, S):
    return np.all(np.abs(x - y) <= 2 * (1e-9 * max(1.0, S / 3.0) + 1e-13 * np.abs(y)))


def solute_sums_match(bs, no, du, ovl, b0, n0):
    hb, hn = common.widom_host_sums(du, ovl, b0, n0, T)
    assert np.array_equal(no, hn), (no, hn)
    assert np.all((bs == hb) | (np.abs(bs - hb) <= 1e-14 * np.abs(hb))), (bs, hb)


def pair_sums_match(sm, du, fl, sums0, temperature=T):
    hs = pr.host_sums(du, fl, sums0, temperature)
    for k in SUMS[1::2]:
        assert np.array_equal(sm[k], hs[k]), (k, sm[k], hs[k])
    for k in SUMS[0::2]:
        assert np.all((sm[k] == hs[k]) | (np.abs(sm[k] - hs[k]) <= 1e-14 * np.abs(hs[k]))), (k, sm[k], hs[k])


def start_sums(b, K, seed=11):
    s = b.pair_sums(None, K)
    r = np.random.default_rng(seed)
    for k in SUMS[0::2]:
        s[k][...] = r.random(s[k].shape) * 1e-3
    for k in SUMS[1::2]:
        s[k][...] = r.integers(0, 5, size=s[k].shape)
    return s


def sentinels(b, K):
    s = b.pair_sums(None, K)
    for k in SUMS[0::2]:
        s[k][...] = 7.5
    for k in SUMS[1::2]:
        s[k][...] = 3
    return s


def untouched(s):
    return all(np.all(s[k] == 7.5) for k in SUMS[0::2]) and all(np.all(s[k] == 3) for k in SUMS[1::2])


def check_solute_all(so, b, mol, du, ovl, what=""):
    return [sr.check_solute(so, b, r, mol[r], du[r], ovl[r], what=what, cache=False) for r in range(b.R)]


def check_pair_all(po, b, mol_a, mol_b, du, fl, what=""):
    out = [pr.check_pair(po, b, r, mol_a[r], mol_b[r], du[r], fl[r], what=what, cache=False) for r in range(b.R)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


# ---- 1. separate cutoffs ------------------------------------------------------------------------
@pytest.mark.parametrize("lj,qq", [(8.0, 10.0), (10.0, 8.0)])
def test_separate_cutoffs(lj, qq, cfg4, orc):
    """LJ and Coulomb cutoffs apart: random insertions of a solute and of a pair; the solute's
    reference point at +-1e-12 relative of each gate around foreign COMs; B at +-1e-12 relative of
    each gate from A, where between the gates exactly one of x_lj and x_real is zero."""
    a = cfg4
    L = float(a["box"])
    sol, pair = pr.path_solute(a), pr.path_pair(a)
    so, po = sr.SoluteOracle(orc, a, sol, lj, qq), pr.PairOracle(orc, a, pair, lj, qq)
    b = make_batch(a, 2, lj, qq)
    try:
        b.set_option("device_moves", 1)
        b.run(60, T, 0.3, 0.2, seed=99)
        # (a) random insertions
        _, _, mol, du, ovl = b.widom_solute(sol, 8, T, seed=31, outputs=True)
        check_solute_all(so, b, mol, du, ovl, what=(lj, qq))
        sm, ma, mb, pdu, fl = b.widom_pair(pair, pr.PATH_D, 6, T, seed=32, outputs=True)
        ref, _ = check_pair_all(po, b, ma, mb, pdu, fl, what=(lj, qq))
        assert np.abs(ref[:, :, 0, 0]).max() > 1.0 and (ref[:, :, 6:10, :2] != 0).any()
        pair_sums_match(sm, pdu, fl, b.pair_sums(None, 5))
        # (b) the solute on either side of each gate of two waters
        mols = np.array([sr.gate_cases(b.get_replica(r)[0], L, sol, lj, qq)[0] for r in range(2)])
        assert mols.shape[1] == 24
        bs, no, du, ovl = b.widom_solute_at(sol, mols, T)
        check_solute_all(so, b, mols, du, ovl, what=(lj, qq, "gates"))
        solute_sums_match(bs, no, du, ovl, np.zeros(2), np.zeros(2, dtype=np.int64))
        # (c) B on either side of each gate of A
        mol_a = np.ascontiguousarray(ma[:, :3])
        mol_b = np.array([pr.pair_gate_cases(mol_a[r], L, pair, lj, qq, seed=17 + r) for r in range(2)])
        sm, pdu, fl = b.widom_pair_at(pair, mol_a, mol_b, T)
        check_pair_all(po, b, mol_a, mol_b, pdu, fl, what=(lj, qq, "A-B gates"))
        for r in range(2):
            assert pr.gate_pattern(pdu[r, :, 5:], lj, qq), pdu[r, :, 5:, :2]
        assert np.all(pdu[:, :, 5:, 2] != 0.0)
    finally:
        b.close()


# ---- 2. site counts -----------------------------------------------------------------------------
@pytest.mark.parametrize("S", [4, 5])
def test_charged_solutes_at_the_table_switch(S, cfg4, two, orc):
    """Charged solutes of 4 sites (k_solute_wave<4>) and of 5 (k_solute_wave<16>)."""
    b = two
    sol = sr.synthetic(cfg4, S, seed=S)
    assert np.count_nonzero(sol.charge) == S
    bs, no, mol, du, ovl = b.widom_solute(sol, 12, T, seed=60 + S, draw0=2, outputs=True)
    assert mol.shape == (2, 12, S + 1, 3)
    check_solute_all(sr.SoluteOracle(orc, cfg4, sol, RC, RC), b, mol, du, ovl, what=S)
    assert np.all(du[:, :, 2] != 0.0)
    solute_sums_match(bs, no, du, ovl, np.zeros(2), np.zeros(2, dtype=np.int64))
    _, _, du2, ovl2 = b.widom_solute_at(sol, mol, T)
    assert same((du, ovl), (du2, ovl2))


@pytest.mark.parametrize("SA,SB", [(15, 1), (1, 15), (8, 8)])
def test_pair_site_counts(SA, SB, cfg4, two, orc):
    """A 15-site solute fills its slot of the tile to the last word; 8 x 8 sites keep all 64 lanes of
    the A-B term busy (a cross table without a zeroed entry)."""
    b = two
    pair = pr.full_pair(cfg4, 8, 8) if (SA, SB) == (8, 8) else pr.synthetic_pair(cfg4, SA, SB)
    d = (3.0, 5.0, 7.0, 11.0)
    sm, ma, mb, du, fl = b.widom_pair(pair, d, 4, T, seed=70 + SA, draw0=1, outputs=True)
    assert ma.shape == (2, 4, SA + 1, 3) and mb.shape == (2, 4, 4, SB + 1, 3)
    ref, _ = check_pair_all(pr.PairOracle(orc, cfg4, pair), b, ma, mb, du, fl, what=(SA, SB))
    assert np.all(du[:, :, 5:, 2] != 0.0) and np.abs(ref[:, :, 5:8, :2]).max() > 0
    if (SA, SB) == (8, 8):
        xpar = np.stack([pair.eps_ab, pair.sig_ab, pair.a.charge[:, None] * pair.b.charge[None, :]], axis=2)
        assert xpar.shape == (8, 8, 3) and np.all(xpar != 0.0) and np.all(pair.eps_ab > 0.001)
        assert np.any(du[:, :, 5:8, 0] != 0.0) and np.any(du[:, :, 5:8, 1] != 0.0)
    pair_sums_match(sm, du, fl, b.pair_sums(None, 4))
    sm2, du2, fl2 = b.widom_pair_at(pair, ma, mb, T)
    assert same((sm, du, fl), (sm2, du2, fl2))
    if (SA, SB) == (15, 1):
        # A and B swapped, placements swapped (one separation at a time): dA and dB change places, x stays
        sw = pair.swapped()
        for k in range(4):
            _, du3, fl3 = b.widom_pair_at(sw, np.ascontiguousarray(mb[:, :, k]), np.ascontiguousarray(ma[:, :, None]), T)
            for row3, row, S in ((0, 1 + k, SB), (1, 0, SA), (2, 5 + k, SA + SB)):
                assert within_twice(du3[:, :, row3], du[:, :, row], S), (k, row)
            assert np.array_equal(fl3[:, :, 0] & 1, fl[:, :, 1 + k] & 1)
            assert np.array_equal(fl3[:, :, 1] & 5, (fl[:, :, 0] & 1) | (fl[:, :, 1 + k] & 4))


@pytest.mark.parametrize("methane_first", [True, False])
def test_a_pair_with_one_uncharged_solute(methane_first, cfg4, two, orc):
    """Methane with a dipole, in both orders: k_solute_pair_wave<16> with one solute's phase rows all
    zero and q_a q_b = 0 throughout.  The uncharged solute's real and recip entries are 0.0, so is
    every x real and recip, and the dipole's terms are widom_solute's of the same placements."""
    b = two
    pair = pr.mixed_pair(cfg4, methane_first)
    dip = pair.b if methane_first else pair.a
    d = (3.0, 4.5, 6.5, 11.0)
    sm, ma, mb, du, fl = b.widom_pair(pair, d, 6, T, seed=75, draw0=3, outputs=True)
    check_pair_all(pr.PairOracle(orc, cfg4, pair), b, ma, mb, du, fl, what=pair)
    assert np.all(du[:, :, 5:, 1:] == 0.0) and np.all(du[:, :, 5:8, 0] != 0.0) and np.all(du[:, :, 8, 0] == 0.0)
    if methane_first:
        assert np.all(du[:, :, 0, 1:] == 0.0) and np.all(du[:, :, 0, 0] != 0.0)
        for k in range(4):
            _, _, sdu, sov = b.widom_solute_at(dip, np.ascontiguousarray(mb[:, :, k]), T)
            assert within_twice(du[:, :, 1 + k], sdu, 2), k
            assert np.array_equal(fl[:, :, 1 + k] & 1, sov & 1)
        assert np.all(du[:, :, 1:5, 2] != 0.0)
    else:
        assert np.all(du[:, :, 1:5, 1:] == 0.0) and np.all(du[:, :, 1:5, 0] != 0.0)
        _, _, smol, sdu, sov = b.widom_solute(dip, 6, T, seed=75, draw0=3, outputs=True)
        assert same(ma, smol) and within_twice(du[:, :, 0], sdu, 2)
        assert np.array_equal(fl[:, :, 0] & 1, sov & 1) and np.all(du[:, :, 0, 2] != 0.0)
    pair_sums_match(sm, du, fl, b.pair_sums(None, 4))


# ---- 3. separation counts -----------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 7, 32])
def test_separation_counts(K, cfg4, two, orc):
    """K = 1 (two placements, one short tile), 7 (two full tiles, the second without A) and 32 =
    MMC_PAIR_MAX_SEP (nine tiles, the last of one placement): every row against the oracle; A's row
    and separation k's rows within twice the tolerance of a K = 1 call at d[k] with the same draws
    (only the tiling differs); the same bytes for every launch shape."""
    b = two
    R, M = 2, 4
    pair = pr.path_pair(cfg4)
    SA, SB = pair.a.n_sites, pair.b.n_sites
    d = pr.separations(K)
    runs = []
    for wgs in (0, 1, 2):
        b.set_option("wave_wgs", wgs)
        runs.append(b.widom_pair(pair, d, M, T, seed=33, draw0=1, sums=start_sums(b, K), outputs=True))
    b.set_option("wave_wgs", 0)
    sm, ma, mb, du, fl = runs[0]
    assert du.shape == (R, M, 1 + 2 * K, 3) and fl.shape == (R, M, 1 + K) and mb.shape == (R, M, K, SB + 1, 3)
    for other in runs[1:]:
        assert same(runs[0], other)
    check_pair_all(pr.PairOracle(orc, cfg4, pair), b, ma, mb, du, fl, what=K)
    pair_sums_match(sm, du, fl, start_sums(b, K))
    for k in range(K):
        _, a1, b1, d1, f1 = b.widom_pair(pair, (d[k],), M, T, seed=33, draw0=1, outputs=True)
        assert same(a1, ma) and same(b1[:, :, 0], np.ascontiguousarray(mb[:, :, k])), k
        for row1, row, S in ((0, 0, SA), (1, 1 + k, SB), (2, 1 + K + k, SA + SB)):
            assert within_twice(d1[:, :, row1], du[:, :, row], S), (k, row)
        assert np.array_equal(f1[:, :, 0], fl[:, :, 0]) and np.array_equal(f1[:, :, 1], fl[:, :, 1 + k]), k


@pytest.mark.parametrize("K", [0, 33])
def test_separation_counts_refused(K, cfg4, two):
    b = two
    pair = pr.path_pair(cfg4)
    d = np.linspace(2.5, 14.9, K)
    s = sentinels(b, K)
    with pytest.raises(_lib.MMCError) as ei:
        b.widom_pair(pair, d, 4, T, 1, sums=s)
    assert ei.value.status == _lib.MMC_ERR_ARG and "n_sep" in str(ei.value) and untouched(s)
    s = sentinels(b, K)
    with pytest.raises(_lib.MMCError) as ei:
        b.widom_pair_at(pair, np.full((2, 2, 4, 3), 5.0), np.full((2, 2, K, 5, 3), 6.0), T, sums=s)
    assert ei.value.status == _lib.MMC_ERR_ARG and "n_sep" in str(ei.value) and untouched(s)


# ---- 4. small systems ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", pr.SMALL_N)
def test_small_systems(n, cfg4, orc):
    """The first n molecules of configuration 4 in its 30 A box, no moves: below one wave, at +-1 of
    64 and of 256 (the scans walk in trips of 256 with the index clamped to n - 1).  Random insertions
    and _at placements 3 A from molecule n - 1."""
    a = sr.first_molecules(cfg4, n)
    sol, pair = pr.path_solute(cfg4), pr.path_pair(cfg4)
    so, po = sr.SoluteOracle(orc, a, sol, RC, RC), pr.PairOracle(orc, a, pair)
    b = make_batch(a, 2)
    try:
        assert b.n_mol == n
        bs, no, mol, du, ovl = b.widom_solute(sol, 4, T, seed=40 + n, outputs=True)
        check_solute_all(so, b, mol, du, ovl, what=n)
        solute_sums_match(bs, no, du, ovl, np.zeros(2), np.zeros(2, dtype=np.int64))
        sm, ma, mb, pdu, fl = b.widom_pair(pair, pr.PATH_D, 4, T, seed=41 + n, outputs=True)
        check_pair_all(po, b, ma, mb, pdu, fl, what=n)
        pair_sums_match(sm, pdu, fl, b.pair_sums(None, 5))
        m1, ma1, mb1 = (np.repeat(x, 2, axis=0) for x in pr.small_cases(a, n, sol, pair))
        bs, no, du, ovl = b.widom_solute_at(sol, m1, T)
        check_solute_all(so, b, m1, du, ovl, what=(n, "at"))
        sm, pdu, fl = b.widom_pair_at(pair, ma1, mb1, T)
        check_pair_all(po, b, ma1, mb1, pdu, fl, what=(n, "at"))
        assert np.all(np.isfinite(du)) and np.all(np.isfinite(pdu))
        if n >= 2:
            assert du[0, 0, 0] != 0.0 and pdu[0, 0, 0, 0] != 0.0
        assert same(du[0], du[1]) and same(pdu[0], pdu[1])
    finally:
        b.close()


# ---- 5. after every path that changes the committed state ---------------------------------------
def both_all(orc, a, b, seed, what, rc=RC, alpha=5.6, d=pr.PATH_D):
    """One widom_solute call (5 sites) and one widom_pair call (K = 5) on every replica against the
    oracle at get_boxes(), and their sums against the host's reduction."""
    sol, pair = pr.path_solute(a), pr.path_pair(a)
    bs, no, mol, du, ovl = b.widom_solute(sol, 4, T, seed=seed, outputs=True)
    check_solute_all(sr.SoluteOracle(orc, a, sol, rc, rc, alpha), b, mol, du, ovl, what=what)
    solute_sums_match(bs, no, du, ovl, np.zeros(b.R), np.zeros(b.R, dtype=np.int64))
    sm, ma, mb, pdu, fl = b.widom_pair(pair, d, 4, T, seed=seed + 100, outputs=True)
    check_pair_all(pr.PairOracle(orc, a, pair, rc, rc, alpha), b, ma, mb, pdu, fl, what=what)
    pair_sums_match(sm, pdu, fl, b.pair_sums(None, len(d)))


def test_after_host_decided_runs(cfg4, orc):
    """One step per launch, the host decides (persistent = 0, accept_on_device = 0)."""
    with make_batch(cfg4, 8) as b:
        for k, v in (("device_moves", 1), ("kernel", 2), ("persistent", 0), ("accept_on_device", 0)):
            b.set_option(k, v)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        e, st = b.run(37, T, 0.3, 0.2, seed=5, energies=e)
        assert st["device_decisions"] == 0 and st["trans_accept"] + st["rot_accept"] > 0
        both_all(orc, cfg4, b, 40, "host-decided")


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
        both_all(orc, cfg4, b, 41, per_launch)
        for x, k in ((b, 0), (tw, 1)):
            es[k], _ = x.run(2 * per_launch + 3, T, 0.3, 0.2, seed=7, energies=es[k], n_groups=2, n_parts=1)
        assert es[0].tobytes() == es[1].tobytes()
        for r in range(R):
            assert same(b.get_replica(r), tw.get_replica(r)), r


def test_after_the_latency_server(cfg4, orc):
    """One replica with the default options: the latency server runs the chain."""
    with make_batch(cfg4, 1) as b:
        b.set_option("device_moves", 1)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        e, st = b.run(150, T, 0.3, 0.2, seed=8, energies=e, n_groups=1)
        assert st["server_steps"] == 150
        both_all(orc, cfg4, b, 42, "latency")


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
        both_all(orc, a, b, 43, "eval/settle")


def test_volume_trial_accept_and_reject(cfg4, orc):
    """One replica: between mmc_batch_volume_trial and its decision all four calls are refused and
    write nothing; after a reject they give the same bytes as before the trial; after an accept the
    terms in the new box (get_boxes, kappa = 5.6 / box), and a separation that fitted half the old
    box is refused."""
    a = cfg4
    sol, pair = pr.path_solute(a), pr.path_pair(a)
    L1 = (0.99 * a["box"] ** 3) ** (1 / 3)
    assert 14.97 < a["box"] / 2 and 14.97 > L1 / 2 > RC
    with make_batch(a, 1) as b:
        b.set_option("device_moves", 1)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        b.run(80, T, 0.3, 0.2, seed=9, energies=e, n_groups=1)

        def calls():
            out = [b.widom_solute(sol, 8, T, seed=44, outputs=True),
                   b.widom_pair(pair, pr.PATH_D, 8, T, seed=45, outputs=True)]
            out.append(b.widom_solute_at(sol, out[0][2], T))
            out.append(b.widom_pair_at(pair, out[1][1], out[1][2], T))
            return out

        before = calls()
        mols = (before[0][2], before[1][1], before[1][2])
        far = b.widom_pair(pair, (14.97,), 2, T, 1)
        assert np.all(np.isfinite(far["boltz_ab"]))
        for accept in (False, True):
            b.volume_trial(L1, 5.6 / L1)
            s, bs, no = sentinels(b, 5), np.full(1, 7.5), np.full(1, 3, dtype=np.int64)
            for call in (lambda: b.widom_solute(sol, 4, T, 1, boltz_sum=bs, n_overlap=no),
                         lambda: b.widom_solute_at(sol, mols[0], T, boltz_sum=bs, n_overlap=no),
                         lambda: b.widom_pair(pair, pr.PATH_D, 4, T, 1, sums=s),
                         lambda: b.widom_pair_at(pair, mols[1], mols[2], T, sums=s)):
                with pytest.raises(_lib.MMCError) as ei:
                    call()
                assert ei.value.status == _lib.MMC_ERR_STATE and bs[0] == 7.5 and no[0] == 3 and untouched(s)
            if accept:
                b.volume_accept()
            else:
                b.volume_reject()
                assert same(before, calls())
        assert b.get_boxes()[0] == L1
        both_all(orc, a, b, 46, "volume accept")
        s = sentinels(b, 1)
        with pytest.raises(_lib.MMCError) as ei:
            b.widom_pair(pair, (14.97,), 2, T, 1, sums=s)
        assert ei.value.status == _lib.MMC_ERR_ARG and "half the box" in str(ei.value) and untouched(s)


def test_after_run_npt(cfg4, orc):
    """mmc_batch_run_npt on one replica: the terms at the final box of get_boxes()."""
    a = cfg4
    with make_batch(a, 1) as b:
        b.set_option("device_moves", 1)
        e0 = float(b.potential_ewald(as_array=True)["energy"][0])
        e1, st, ns = b.run_npt(8, T, 0.03, 0.05 * a["box"] ** 3, 0.3, 0.2, 13, e0, moves_per_sweep=40)
        assert ns["vol_attempt"] == 8
        both_all(orc, a, b, 47, ("npt", float(b.get_boxes()[0]), ns["vol_accept"]))


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
        both_all(orc, a, b, 48, "set_replica")


@pytest.mark.parametrize("mode", [1, 2])
def test_after_quaternion_chains(mode, orc):
    """200 steps of the quaternion route on 216 molecules in 18.7 A at r_cut 7 (mode 1 deforms the
    molecules, mode 2 does not), then both calls."""
    from test_gpu_replay_paths import Q_RCUT, system
    a, quat, db = system("q216", mode == 1)
    assert max(pr.SMALL_D) < a["box"] / 2
    with make_batch(a, 2, Q_RCUT, Q_RCUT) as b:
        b.set_option("device_moves", 1)
        b.set_orientations(quat, db, faithful=mode == 1)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        b.run(200, T, 0.3, 0.3, seed=77, energies=e)
        both_all(orc, a, b, 49, mode, rc=Q_RCUT, d=pr.SMALL_D)


def test_tip3p_lattice(orc):
    """The 216-water TIP3P deck lattice (box 18.69 A, r_cut 9, alpha 5.5) after 100 steps."""
    a = sr.tip3p_lattice()
    assert max(pr.SMALL_D) < a["box"] / 2
    with make_batch(a, 2, sr.MEA_RCUT, sr.MEA_RCUT, alpha=sr.MEA_ALPHA) as b:
        b.set_option("device_moves", 1)
        b.run(100, T, 0.3, 0.2, seed=10)
        both_all(orc, a, b, 50, "tip3p", rc=sr.MEA_RCUT, alpha=sr.MEA_ALPHA, d=pr.SMALL_D)


# ---- 6. flags in the later blocks of k_pair_reduce ----------------------------------------------
def test_flagged_insertions_in_later_blocks(cfg4, three, orc):
    """200 caller-given insertions per replica, K = 3, with an overlap and a non-finite dU of A, of a
    B_k and of the A-B term planted in the second and third blocks of 64 (and one in the first),
    solute_pair_ref.flag_plants: the flag bytes are the planted ones (all four bits of every entry
    of every insertion are the oracle's, check_pair with `nonfinite`), the counts and the sums the
    host's from non-zero starting sums, the same bytes for every launch shape.  The A plants also
    through widom_solute_at."""
    a, b = cfg4, three
    R, M, K = b.R, pr.FLAG_M, len(pr.FLAG_D)
    pair = pr.flag_pair(a)
    _, mol_a, mol_b, _, _ = b.widom_pair(pair, pr.FLAG_D, M, T, seed=pr.FLAG_SEED, outputs=True)
    plants = [pr.flag_plants(a, pair, b.get_replica(r)[1], mol_a[r], mol_b[r], r) for r in range(R)]
    runs = []
    for wgs in (0, 1, 2):
        b.set_option("wave_wgs", wgs)
        runs.append(b.widom_pair_at(pair, mol_a, mol_b, T, sums=start_sums(b, K)))
    b.set_option("wave_wgs", 0)
    sm, du, fl = runs[0]
    for other in runs[1:]:
        assert same(runs[0], other)
    po = pr.PairOracle(orc, a, pair)
    for r in range(R):
        assert len(plants[r]) == 7
        for (j, col), byte in plants[r].items():
            assert fl[r, j, col] == byte, (r, j, col, fl[r, j], byte)
        assert np.all(fl[r, 100, 1:] & 8) and np.all(fl[r, [5, 70], 0] == 1)
        # every row of the planted insertions and of their neighbours against the oracle, all four bits
        js = sorted({j for j, _ in plants[r]} | {0, 63, 64, 127, 129, 192, 199})
        nonfinite = []
        pr.check_pair(po, b, r, mol_a[r][js], mol_b[r][js], du[r][js], fl[r][js], what="planted", cache=False,
                      nonfinite=nonfinite)
        # A at 100: row 0; B_2 at 140: row 3; x_2 of the B-on-A plant: row 1 + K + 2
        assert sorted(row for _, row in nonfinite) == [0, 3, 1 + K + 2], nonfinite
    # the other insertions: finite rows, no bit 1 or 3 unless a term is non-finite
    with np.errstate(invalid="ignore"):
        _, _, _, du_ab = pr.du_total(du)
    assert np.array_equal((fl[:, :, 1:] & 8) != 0, ~np.isfinite(du_ab))
    assert np.count_nonzero(~np.isfinite(du_ab)) == R * (K + 1 + 1)
    pair_sums_match(sm, du, fl, start_sums(b, K))
    s0 = start_sums(b, K)
    assert np.all(sm["n_zero_ab"] - s0["n_zero_ab"] >= 3) and np.all(sm["n_zero_a"] - s0["n_zero_a"] >= 3)
    # the A plants as single solutes
    js = [5, 70, 100]
    mols = np.ascontiguousarray(mol_a[:, js])
    b0, n0 = np.array([0.25, 0.0, 3.0]), np.array([1, 2, 0], dtype=np.int64)
    bs, no, sdu, sov = b.widom_solute_at(pair.a, mols, T, boltz_sum=b0.copy(), n_overlap=n0.copy())
    assert np.array_equal(sov, np.tile(np.array([1, 1, 2], dtype=np.uint8), (R, 1)))
    so = sr.SoluteOracle(orc, a, pair.a, RC, RC)
    for r in range(R):
        nonfinite = []
        sr.check_solute(so, b, r, mols[r], sdu[r], sov[r], what="planted A", cache=False, nonfinite=nonfinite)
        assert nonfinite == [2]
    assert np.array_equal(no, n0 + 3) and np.array_equal(bs, b0)


def test_an_overlapping_a_weighs_nothing_in_block_two(cfg4, three, orc):
    """w_AB = 0 under A's flag alone, where it shows: M = 65 puts a single insertion into the second
    block of k_pair_reduce, and that one (and insertion 10) is a dipole whose LJ-free negative site
    overlaps a water H while its dU stays moderate (solute_pair_ref.light_overlap), with a ghost B
    (no flag of the entry's own) at 5000 K: without A's flag the insertion would add a weight far
    above the 1e-14 of the sums' check, asserted here from the returned dU."""
    a, b = cfg4, three
    R, M, K, hot = b.R, pr.HOT_M, len(pr.HOT_D), pr.HOT_T
    pair = pr.hot_pair(a)
    _, mol_a, mol_b, _, _ = b.widom_pair(pair, pr.HOT_D, M, hot, seed=pr.HOT_SEED, outputs=True)
    js = [10, 64]
    for r in range(R):
        for j in js:
            mol_a[r, j] = pr.light_overlap(a, pair.a, b.get_replica(r)[1], seed=29 + j + r)
    runs = []
    for wgs in (0, 1, 2):
        b.set_option("wave_wgs", wgs)
        runs.append(b.widom_pair_at(pair, mol_a, mol_b, hot, sums=start_sums(b, K)))
    b.set_option("wave_wgs", 0)
    sm, du, fl = runs[0]
    for other in runs[1:]:
        assert same(runs[0], other)
    po = pr.PairOracle(orc, a, pair)
    near = [9, 10, 11, 63, 64]
    for r in range(R):
        nonfinite = []
        pr.check_pair(po, b, r, mol_a[r][near], mol_b[r][near], du[r][near], fl[r][near], what="light overlap",
                      cache=False, nonfinite=nonfinite)
        assert not nonfinite
    assert np.all(fl[:, js, 0] == 1) and not fl[:, js, 1:].any() and np.all(du[:, :, 1:] == 0.0)
    s0 = start_sums(b, K)
    pair_sums_match(sm, du, fl, s0, temperature=hot)
    assert np.all(sm["n_zero_ab"] - s0["n_zero_ab"] >= 2) and not np.any(sm["n_zero_b"] - s0["n_zero_b"])
    # what the planted insertions would have added without A's flag
    w = np.exp(-((du[:, js, 0, 0] + du[:, js, 0, 1]) + du[:, js, 0, 2]) / hot)
    print("weights under the flag:", w, "sums:", sm["boltz_ab"])
    assert np.all(w >= 1e-8 * sm["boltz_ab"].max(1)[:, None]), (w, sm["boltz_ab"])
    unflagged = fl.copy()
    unflagged[:, js, 0] = 0
    alt = pr.host_sums(du, unflagged, s0, hot)
    assert np.all(np.abs(alt["boltz_ab"] - sm["boltz_ab"]) > 1e-10 * sm["boltz_ab"])


# ---- 7. the generator ---------------------------------------------------------------------------
def test_generated_placements_against_the_mirror(cfg4, three):
    """widom_pair's and widom_solute's generated placements against observables.pair_molecules /
    solute_molecules with the Philox counter draw0 + j crossing 2^32, separations of which many wrap
    (precondition in test_solute_paths_host.py); insertion j depends on (seed, draw0 + j) alone."""
    from metropolismontecarlo_amd.device import philox4x32
    b = three
    L = b.box
    pair = pr.path_pair(cfg4)
    d, seed, draw0, M = pr.GEN_D, pr.GEN_SEED, pr.GEN_DRAW0, pr.GEN_M
    assert draw0 < 2 ** 32 <= draw0 + M - 1
    out = b.widom_pair(pair, d, M, T, seed=seed, draw0=draw0, outputs=True)
    _, ma, mb, du, fl = out
    for r in (0, b.R - 1):
        ra, rb = obs.pair_molecules(philox4x32, seed, draw0, M, r, L, pair.a.offsets, pair.b.offsets, d)
        assert np.abs(ma[r] - ra).max() <= 1e-12 and np.abs(mb[r] - rb).max() <= 1e-12, r
    ca, cb = ma[:, :, None, -1], mb[:, :, :, -1]
    assert np.all((cb >= 0) & (cb <= L))
    sep = cb - ca
    sep = sep + common.image_shift(sep, L)
    assert np.abs(np.linalg.norm(sep, axis=3) - np.array(d)).max() <= 1e-12
    later = b.widom_pair(pair, d, 5, T, seed=seed, draw0=2 ** 32, outputs=True)
    assert same([np.ascontiguousarray(x[:, 3:]) for x in out[1:]], later[1:])
    sol = pr.path_solute(cfg4)
    out = b.widom_solute(sol, M, T, seed=seed, draw0=draw0, outputs=True)
    for r in (0, b.R - 1):
        ref = obs.solute_molecules(philox4x32, seed, draw0, M, r, L, sol.offsets)
        assert np.abs(out[2][r] - ref).max() <= 1e-12, r
    later = b.widom_solute(sol, 5, T, seed=seed, draw0=2 ** 32, outputs=True)
    assert same([np.ascontiguousarray(x[:, 3:]) for x in out[2:]], later[2:])


# ---- 8. the shared scratch ----------------------------------------------------------------------
def test_shared_scratch_between_layouts(cfg4):
    """Calls of different scratch layouts in a row on one batch -- among them a pair call whose device
    and pinned scratch grow -- each bit for bit what the same call makes on a fresh batch."""
    a = cfg4
    pair, sol = pr.path_pair(a), pr.path_solute(a)
    d2, d32 = (3.0, 6.0), pr.separations(32)
    mols = {}

    def pair_again(b):
        out = b.widom_pair(pair, d2, 4, T, seed=86, draw0=2, sums=start_sums(b, 2), outputs=True)
        mols["a"], mols["b"] = out[1], out[2]
        return out

    calls = (
        lambda b: b.widom_pair(pair, d2, 4, T, seed=81, sums=start_sums(b, 2), outputs=True),
        lambda b: b.widom_pair(pair, d32, 40, T, seed=82, sums=start_sums(b, 32), outputs=True),
        lambda b: b.widom_solute(sol, 4, T, seed=83, boltz_sum=np.full(3, 0.5), outputs=True),
        lambda b: b.widom(4, T, seed=84, boltz_sum=np.full(3, 0.5), outputs=True),
        lambda b: b.forces(details=True),
        lambda b: b.deletion(T, details=True),
        pair_again,
        lambda b: b.widom_pair_at(pair, mols["a"], mols["b"], T, sums=start_sums(b, 2)),
    )
    with make_batch(a, 3) as b:
        got = [call(b) for call in calls]
    assert same(got[6][3:], got[7][1:])
    for i, (call, g) in enumerate(zip(calls, got)):
        with make_batch(a, 3) as f:
            assert same(g, call(f)), i
