"""CPU preconditions of tests/test_gpu_solute_paths.py, by the oracle alone on the starting
configuration: what keeps a GPU test there from passing vacuously -- the gates do switch terms, the
planted placements are flagged as intended, the generated B placements do wrap, the rows of the long
separation lists are not trivially zero, the small systems give finite terms."""
import numpy as np
import pytest

import common
import solute_pair_ref as pr
import solute_ref as sr
from metropolismontecarlo_amd import observables as obs
from metropolismontecarlo_amd.device import philox4x32

CUTOFFS = [(8.0, 10.0), (10.0, 8.0)]


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def cfg4():
    return common.nist_arrays(4, "unwrapped")


def start(a):
    return np.asarray(a["com"], dtype=float), np.asarray(a["coords"], dtype=float), float(a["box"])


@pytest.mark.parametrize("lj,qq", CUTOFFS)
def test_the_pair_gates_switch_one_term_each(orc, cfg4, lj, qq):
    """Item 1(c): inside both gates neither x term is zero, outside both are, between them exactly one."""
    com, coords, L = start(cfg4)
    pair = pr.path_pair(cfg4)
    po = pr.PairOracle(orc, cfg4, pair, lj, qq)
    mol_a, _ = obs.pair_molecules(philox4x32, 32, 0, 3, 0, L, pair.a.offsets, pair.b.offsets, (3.0,))
    mol_b = pr.pair_gate_cases(mol_a, L, pair, lj, qq)
    assert mol_b.shape == (3, 4, pair.b.n_sites + 1, 3)
    x = np.array([[po.x_terms(mol_a[i], mol_b[i, k], L)[:3] for k in range(4)] for i in range(3)])
    assert pr.gate_pattern(x, lj, qq), x[:, :, :2]
    zeros = (x[:, 1:3, :2] == 0.0).sum(2)
    assert np.all(zeros == 1) and np.all(x[:, :, 2] != 0.0)


@pytest.mark.parametrize("lj,qq", CUTOFFS)
def test_the_solute_gates_switch_the_oracles_terms(orc, cfg4, lj, qq):
    """Item 1(b): for each gate, stepping from (1 - 1e-12) g to (1 + 1e-12) g changes the oracle's term
    of that gate (lj for the LJ gate, real for the Coulomb gate) in at least two cases."""
    com, coords, L = start(cfg4)
    sol = pr.path_solute(cfg4)
    so = sr.SoluteOracle(orc, cfg4, sol, lj, qq)
    mols, tags = sr.gate_cases(com, L, sol, lj, qq)
    t = {tag: so.terms(com, coords, m, L, key="start") for m, tag in zip(mols, tags)}
    for gi in (0, 1):
        changed = sum(t[(j, gi, di, True)][gi] != t[(j, gi, di, False)][gi]
                      for (j, g, di, inside) in tags if g == gi and inside)
        assert changed >= 2, (gi, changed)


def test_the_planted_placements_are_flagged_as_intended(orc, cfg4):
    """Item 6: the oracle's statement of every planted placement."""
    com, coords, L = start(cfg4)
    pair = pr.flag_pair(cfg4)
    po = pr.PairOracle(orc, cfg4, pair)
    K = len(pr.FLAG_D)
    mol_a, mol_b = obs.pair_molecules(philox4x32, pr.FLAG_SEED, 0, pr.FLAG_M, 0, L, pair.a.offsets, pair.b.offsets,
                                      pr.FLAG_D)
    plant = pr.flag_plants(cfg4, pair, coords, mol_a, mol_b)
    assert sorted(set(plant.values())) == [1, 2, 4, 8, 10] and len(plant) == 7
    assert sum(j < 64 for j, _ in plant) == 1 and sum(64 <= j < 128 for j, _ in plant) >= 2
    assert sum(128 <= j < 192 for j, _ in plant) >= 3
    for (j, col), byte in plant.items():
        rows, ofl = po.reference(com, coords, mol_a[j], mol_b[j], L, key="start")
        want = pr.expected_flags(rows, ofl)
        assert want[col] == byte, (j, col, want, byte)
        with np.errstate(invalid="ignore"):
            du_a, du_b, x, du_ab = pr.du_total(rows)
        if col == 0:
            assert np.isfinite(du_a) == (byte == 1)
            if byte == 2:
                assert np.all(want[1:] & 8)         # dU_AB of every separation goes with dU_A
        elif byte == 8:                             # B on A: no overlap anywhere, x_lj non-finite alone
            assert not ofl[col] and not ofl[0] and not np.isfinite(rows[K + col, 0])
            assert np.isfinite(du_a) and np.isfinite(du_b[col - 1])
        elif byte == 4:                             # the A-B overlap: everything finite
            assert ofl[col] == 4 and np.isfinite(du_a) and np.isfinite(du_b[col - 1]) and np.isfinite(du_ab[col - 1])
        elif byte == 1:
            assert np.isfinite(du_b[col - 1]) and rows[col, 1] == 0.0
        else:
            assert not np.isfinite(du_b[col - 1]) and not ofl[col]
    # the A plants as single solutes
    so = sr.SoluteOracle(orc, cfg4, pair.a, pr.RCUT, pr.RCUT)
    for j, byte in ((5, 1), (70, 1), (100, 2)):
        lj, real, recip, ov = so.terms(com, coords, mol_a[j], L, key="start")
        assert ov == (byte == 1) and bool(np.isfinite(lj + real + recip)) == (byte == 1)


def test_the_light_overlap_would_weigh_something(orc, cfg4):
    """Item 6, w_AB = 0 under A's flag: the oracle flags the dipole of solute_pair_ref.light_overlap as
    an overlap, its dU is finite, and at HOT_T the weight exp(-dU / T) it would have without the flag
    is above 1e-3 -- against sums of at most a few thousand (65 insertions of weight <= exp(3): dU
    >= -15000 K for a dipole of 0.45 e), a share far above the 1e-14 the sums are checked to."""
    com, coords, L = start(cfg4)
    sol = pr.hot_pair(cfg4).a
    so = sr.SoluteOracle(orc, cfg4, sol, pr.RCUT, pr.RCUT)
    for seed in (29, 30, 93):
        lj, real, recip, ov = so.terms(com, coords, pr.light_overlap(cfg4, sol, coords, seed), L, key="start")
        assert ov and real == 0.0 and np.isfinite(lj + recip)
        assert -15000.0 < lj + recip and np.exp(-(lj + recip) / pr.HOT_T) > 1e-3, (seed, lj, recip)


def test_the_generated_b_placements_wrap(cfg4):
    """Item 7: among the mirror's placements for the GPU test's draws at least a third of the c_B are
    wrapped on some axis, in both directions."""
    L = float(cfg4["box"])
    pair = pr.path_pair(cfg4)
    n = up = down = total = 0
    for r in (0, 2):
        ma, mb = obs.pair_molecules(philox4x32, pr.GEN_SEED, pr.GEN_DRAW0, pr.GEN_M, r, L, pair.a.offsets,
                                    pair.b.offsets, pr.GEN_D)
        raw = ma[:, None, -1] + (mb[:, :, -1] - ma[:, None, -1] + common.image_shift(mb[:, :, -1] - ma[:, None, -1], L))
        assert np.all((mb[:, :, -1] >= 0) & (mb[:, :, -1] <= L))
        total += raw.shape[0] * raw.shape[1]
        n += np.count_nonzero(((raw > L) | (raw < 0)).any(2))
        up += np.count_nonzero(raw > L)
        down += np.count_nonzero(raw < 0)
    assert 3 * n >= total and up > 0 and down > 0, (n, total, up, down)


@pytest.mark.parametrize("K", [7, 32])
def test_the_long_separation_lists_are_not_trivial(orc, cfg4, K):
    """Item 3: the oracle's lj term is non-zero for A and for at least half of the separations of every
    insertion of replica 0's draws; every separation has a non-zero x recip term."""
    com, coords, L = start(cfg4)
    pair = pr.path_pair(cfg4)
    po = pr.PairOracle(orc, cfg4, pair)
    d = pr.separations(K)
    assert len(d) == K and d[0] == 2.5 and d[-1] == 14.9
    ma, mb = obs.pair_molecules(philox4x32, 33, 1, 4, 0, L, pair.a.offsets, pair.b.offsets, d)
    for j in range(4):
        rows, _ = po.reference(com, coords, ma[j], mb[j], L, key="start")
        assert rows[0, 0] != 0.0 and 2 * np.count_nonzero(rows[1:1 + K, 0]) >= K
        assert np.all(rows[1 + K:, 2] != 0.0)


@pytest.mark.parametrize("n", pr.SMALL_N)
def test_the_small_systems_give_finite_terms(orc, cfg4, n):
    """Item 4: the oracle handles the first n molecules; its terms of the planted _at insertion are
    finite and the lj term is non-zero from two molecules on."""
    a = sr.first_molecules(cfg4, n)
    com, coords, L = start(a)
    assert com.shape == (n, 3) and coords.shape == (3 * n, 3)
    sol, pair = pr.path_solute(cfg4), pr.path_pair(cfg4)
    mol, mol_a, mol_b = pr.small_cases(a, n, sol, pair)
    t = sr.SoluteOracle(orc, a, sol, pr.RCUT, pr.RCUT).terms(com, coords, mol[0, 0], L)
    rows, _ = pr.PairOracle(orc, a, pair).reference(com, coords, mol_a[0, 0], mol_b[0, 0], L)
    assert np.all(np.isfinite(t[:3])) and np.all(np.isfinite(rows))
    if n >= 2:
        assert t[0] != 0.0 and rows[0, 0] != 0.0


def test_the_full_pair_has_no_idle_site_pair(cfg4):
    """Item 2: 64 non-zero eps_ab and 64 non-zero charge products."""
    p = pr.full_pair(cfg4, 8, 8)
    assert np.count_nonzero(p.eps_ab > 0.001) == 64
    assert np.count_nonzero(p.a.charge[:, None] * p.b.charge[None, :]) == 64
    for sa, sb in ((15, 1), (1, 15)):
        q = pr.synthetic_pair(cfg4, sa, sb)
        assert q.a.n_sites == sa and q.b.n_sites == sb and q.a.charge.any() and q.b.charge.any()
    for first in (True, False):
        m = pr.mixed_pair(cfg4, first)
        assert (not m.a.charge.any()) == first and (not m.b.charge.any()) == (not first)
