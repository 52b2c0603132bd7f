"""Host side of tests/test_gpu_wolf_paths.py (no GPU): the Wolf replays of its scenarios on the
CPU oracle, and the conditions under which those scenarios probe what they are meant to -- so that
a fixture or a seed cannot stop probing silently.  Seeds are settled here."""
import numpy as np
import pytest

import common
import test_gpu_wolf_paths as wp
from test_gpu_replay_paths import M_STEPS, Q_RCUT, Q_STEPS, T_STEPS, TINY, system


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def test_replay_wolf_keyword_changes_what_it_says(orc):
    """replay(wolf=True) on 216 molecules: the first step's dU is orc.trial_move's d_lj + d_real of
    the same proposal (the Ewald replay's is d_lj + d_real + d_recip, bit for bit), S(k) is left
    alone, v_acc is there in both styles, and the default is what it was."""
    import test_gpu_replay_paths as rp
    a = system("q216", False)[0]
    e = rp.replay(orc, a, 3, [(30, 777, 0)], 298.15, 0.3, 0.3, Q_RCUT)
    w = rp.replay(orc, a, 3, [(30, 777, 0)], 298.15, 0.3, 0.3, Q_RCUT, wolf=True)
    assert "v_acc" in e and "v_acc" in w
    ew = orc.Ewald(5.6 / a["box"], 5, 27, a["box"])
    s = common.oracle_system(a)
    orc.recip_long(ew, s.coords, s.charge, a["box"])
    assert np.array_equal(w["S"], ew.sumQExpOld) and not np.array_equal(e["S"], ew.sumQExpOld)
    _, c_new, a_new, _, _ = rp.propose(0, 777, 3, 0, s.com[0].copy(), s.coords[:3].copy(), None, None, a["box"],
                                       0.3, 0.3)
    d, _ = orc.trial_move(1, s, ew, Q_RCUT, Q_RCUT, c_new, a_new)
    assert d[2] != 0.0
    assert w["trace"][0][0] == d[0] + d[1] and e["trace"][0][0] == d[0] + d[1] + d[2]
    assert 0 < w["n_acc"] < 30


def test_straddling_system_fails_the_image_condition_on_its_own():
    a, b = system("q216", False)[0], wp.q216_straddling()
    assert Q_RCUT + 2 * wp.r_mol_max(a) + 1e-6 < a["box"] / 2          # q216: IMG = true
    assert not Q_RCUT + 2 * wp.r_mol_max(b) + 1e-6 < b["box"] / 2      # ... and IMG = false
    o = wp.replay_arrays("straddling", wp.MULTI_REPLICA0, ((90, wp.MULTI_SEED),), wp.Q_T, wp.Q_DR, wp.Q_DPHI, Q_RCUT)
    assert 0 < o["n_acc"] < 90


@pytest.mark.parametrize("mode", [1, 2])
def test_quaternion_chains_reject_and_rotate(mode):
    os_ = wp.quat_replays(mode)
    assert sum(Q_STEPS - o["n_acc"] for o in os_.values()) > 20
    assert sum(int(o["n_qrot"].sum()) for o in os_.values()) > 100


def test_window_chains_cross_the_boundary():
    os_ = wp.window_replays()
    hits = [r for r in range(wp.W_R) if os_[r]["crossed"]]
    assert len(hits) >= 3, hits


@pytest.mark.parametrize("n_mol", TINY)
def test_tiny_chains_accept_and_reject(n_mol):
    os_ = wp.tiny_replays(n_mol)
    n_acc = sum(o["n_acc"] for o in os_.values())
    if n_mol == 1:
        assert all(d == 0.0 for o in os_.values() for d, _ in o["trace"])
        assert n_acc == 4 * T_STEPS
    else:
        assert n_acc > 20 and 4 * T_STEPS - n_acc > 5, n_acc


@pytest.mark.parametrize("order", common.MIX_ORDERS)
def test_mixture_chains_move_both_species(order):
    for r, o in wp.mixture_replays(order).items():
        assert all(acc > 0 and rej > 0 for acc, rej in wp.species_counts(order, o)), (order, r)
        assert len(o["trace"]) == M_STEPS


def test_charged_mixture_margin(orc):
    a = wp.charged_mixture()
    assert abs(a["charge"].sum()) > 1.0 and abs(wp.mixture("blocks")["charge"].sum()) < 1e-12
    term, self_ = wp.charged_self_margin(orc)
    assert term > 1e-6 * self_, (term, self_)
    # the oracle's `self` holds the term: its literal double loop and the closed form agree, and
    # differ from the neutral system's constant by it
    s = common.oracle_system(a)
    ew = wp.oracle_ewald(orc, a)
    lit = orc.potential_wolf(s, ew, wp.M_RCUT, wp.M_RCUT, literal_prefactor=True)["self"]
    fast = orc.potential_wolf(s, ew, wp.M_RCUT, wp.M_RCUT, literal_prefactor=False)["self"]
    assert abs(lit - fast) < 1e-9 * abs(fast)
    import math
    neutral = -(math.erfc(ew.kappa * wp.M_RCUT) / 2 / wp.M_RCUT + ew.kappa / math.sqrt(math.pi)) \
        * (a["charge"] ** 2).sum() * ew.factor
    assert abs((fast - neutral) + term) < 1e-9 * abs(fast), (fast, neutral, term)


@pytest.mark.parametrize("n_mol,rho", wp.LONG_SYSTEMS)
def test_long_list_flush_pattern(n_mol, rho):
    flushes = [m[6] for m in wp.scripted_moves(n_mol, rho)]
    assert all(flushes) if n_mol == 2000 else not any(flushes), flushes


# ---- what the GPU tests assert of their replays besides: the chains both accept and reject ---------
@pytest.mark.parametrize("mode", [1, 2])
def test_quaternion_chains_of_several_steps_per_launch_accept_and_reject(mode):
    R, seed, replica0 = wp.QM_R, wp.QM_SEED, wp.QM_REPLICA0
    for r in common.replicas_by_wave_position(R, 2, wave_wgs=1, occ=common.wolf_occ()):
        o = wp.wreplay("q216", mode == 1, replica0 + r, ((Q_STEPS, seed, mode),), wp.Q_T, wp.Q_DR, wp.Q_DPHI, Q_RCUT)
        assert 0 < o["n_acc"] < Q_STEPS, (mode, r)


@pytest.mark.parametrize("n_mol", [17, 18])
def test_tiny_chains_of_eight_steps_per_launch_accept_and_reject(n_mol):
    for r in range(wp.T8_R):
        o = wp.wreplay(f"tiny{n_mol}", False, r, ((wp.T8_STEPS, wp.T8_SEED, 0),), wp.T_T, wp.T_DR, wp.T_DPHI, wp.T_RCUT)
        assert 0 < o["n_acc"] < wp.T8_STEPS, (n_mol, r)


@pytest.mark.parametrize("n_mol", [1, 2])
def test_tiny_quaternion_chains_rotate_the_molecule_just_committed(n_mol):
    n_sub = 0
    for r in range(4):
        o = wp.wreplay(f"tiny{n_mol}", True, wp.TQ_REPLICA0 + r, ((T_STEPS, wp.TQ_SEED0 + n_mol, 1),), wp.T_T, wp.T_DR, wp.T_DPHI, wp.T_RCUT)
        f = [flags for _, flags in o["trace"]]
        n_sub += sum(1 for k in range(1, T_STEPS) if f[k - 1] & 1 and f[k] & 4)
    assert n_sub > 10


def test_rigid_call_after_mode_1_crosses_the_boundary(orc):
    import test_gpu_replay_paths as rp
    a, quat, db = system("window", True)
    n_cross = 0
    for r in range(wp.SWITCH_R):
        o = rp.replay(orc, a, r, [(wp.W_STEPS, wp.SWITCH_SEEDS[0], 1), (wp.W_STEPS, wp.SWITCH_SEEDS[1], 0)], wp.W_T, wp.W_DR, wp.W_DPHI, wp.W_RCUT,
                      quat, db, probe=True, wolf=True)
        n_cross += sum(1 for k in o["crossed"] if k >= wp.W_STEPS)
    assert n_cross > 0


def test_charged_chain_accepts_and_rejects():
    for r in wp.CHECK:
        o = wp.replay_arrays(("charged",), r, ((wp.CHARGED_STEPS, wp.CHARGED_SEED),), wp.M_T, wp.M_DR, wp.M_DPHI,
                             wp.M_RCUT)
        assert 0 < o["n_acc"] < wp.CHARGED_STEPS, r
