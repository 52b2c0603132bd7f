"""CPU tests of parallel tempering's host side: mmc_exchange_round (a pure function: no device, no
batch) against the plain-Python restatement of its header comment (tempering_ref.py), its refusals,
detailed balance on an ensemble whose canonical law is known in closed form, and the helpers of
moves.py, observables.py and sharding.py."""
import numpy as np
import pytest

import tempering_ref
from metropolismontecarlo_amd import _lib, moves, sharding
from metropolismontecarlo_amd import observables as obs
from metropolismontecarlo_amd.device import exchange_round


def _both(n_ladders, n_rungs, parity, seed, replica0, rnd, pressure, e, vol, state, ref_state):
    """One round through the library (numpy state, in place) and the restatement (lists, in place)."""
    temps, rung, attempt, accept = state
    exchange_round(n_rungs, e, temps, rung, seed, rnd, parity=parity, pressure=pressure, volumes=vol,
                   replica0=replica0, attempt=attempt, accept=accept)
    ok = tempering_ref.exchange_round(n_ladders, n_rungs, parity, seed, replica0, rnd, pressure, e.tolist(),
                                      None if vol is None else vol.tolist(), *ref_state)
    assert ok


@pytest.mark.parametrize("n_rungs", [5, 6])
@pytest.mark.parametrize("case", ["nvt", "npt", "inf"])
def test_exchange_round_is_the_restatement_bit_for_bit(n_rungs, case):
    """40 rounds of alternating parity, 7 ladders: temps, rung, attempt and accept equal the
    restatement after every round -- integer for integer, bit for bit.  Energies of order 1e4 K are
    drawn anew every round (as a run between two exchanges would change them); "npt" adds volumes
    and a pressure, "inf" gives one replica the +inf of an overlapping start."""
    n_ladders, seed, replica0, round0 = 7, 0x9E3779B97F4A7C15, 35 * n_rungs, 2 ** 32 - 20   # (crosses a 32-bit word)
    R = n_ladders * n_rungs
    rng = np.random.default_rng(100 + n_rungs)
    ladder = moves.geometric_ladder(260.0, 400.0, n_rungs)
    temps, rung = np.tile(ladder, n_ladders), moves.initial_rungs(R, n_rungs)
    attempt, accept = np.zeros(n_rungs - 1, np.int64), np.zeros(n_rungs - 1, np.int64)
    ref = [temps.tolist(), rung.tolist(), [0] * (n_rungs - 1), [0] * (n_rungs - 1)]
    pressure = 1.5 if case == "npt" else 0.0
    for i in range(40):
        e = -1.0e4 + 4000.0 * rng.standard_normal(R)
        vol = 2.2e4 + 400.0 * rng.standard_normal(R) if case == "npt" else None
        if case == "inf":
            e[(3 * i) % R] = np.inf
        rnd = round0 + i
        _both(n_ladders, n_rungs, rnd & 1, seed, replica0, rnd, pressure, e, vol, (temps, rung, attempt, accept), ref)
        assert temps.tolist() == ref[0] and rung.tolist() == ref[1], i
        assert attempt.tolist() == ref[2] and accept.tolist() == ref[3], i
        assert sorted(temps[:n_rungs].tolist()) == ladder.tolist()       # a swap moves temperatures, it makes none
    # the precondition: the restatement neither always nor never swaps, on any pair of rungs
    ratio = np.array(ref[3]) / np.array(ref[2])
    assert ((ratio > 0.1) & (ratio < 0.9)).all(), ratio
    # an odd round of an even ladder has one pair fewer: 20 rounds of each parity, 7 ladders
    assert ref[2] == [140] * (n_rungs - 1)
    assert np.array_equal(obs.exchange_acceptance(attempt, accept), ratio)


def test_an_infinite_energy_never_swaps():
    n_rungs, R = 4, 8
    temps, rung = np.tile(moves.geometric_ladder(250.0, 500.0, n_rungs), 2), moves.initial_rungs(R, n_rungs)
    e = np.full(R, -9000.0)
    e[1] = e[6] = np.inf              # D would be +inf (a swap "certainly accepted") or NaN
    t0 = temps.copy()
    for rnd in range(6):
        exchange_round(n_rungs, e, temps, rung, 5, rnd)
    assert temps[1] == t0[1] and temps[6] == t0[6] and rung[1] == 1 and rung[6] == 2
    assert (rung[[0, 4]] != [0, 0]).any() or (rung[[3, 7]] != [3, 3]).any()   # equal energies: D = 0, the others do swap


@pytest.mark.parametrize("what", ["rung", "n_rungs", "parity", "temperature"])
def test_exchange_round_refuses_and_changes_nothing(what):
    n_rungs, R = 3, 6
    temps, rung = np.tile([250.0, 300.0, 360.0], 2), moves.initial_rungs(R, n_rungs)
    e = np.array([-5.0, -900.0, -2000.0, -100.0, -50.0, -3000.0])      # every D > 0: a valid call swaps
    kw = dict(n_rungs=n_rungs, parity=0)
    if what == "rung":
        rung[4] = 0                                                   # ladder 1 holds rung 0 twice
    elif what == "n_rungs":
        kw["n_rungs"] = 1
    elif what == "parity":
        kw["parity"] = 2
    else:
        temps[5] = 0.0
    n_cnt = max(kw["n_rungs"] - 1, 0)
    attempt, accept = np.full(n_cnt, 7, np.int64), np.full(n_cnt, 3, np.int64)
    before = temps.copy(), rung.copy()
    with pytest.raises(_lib.MMCError, match="MMC_ERR_ARG"):
        exchange_round(kw["n_rungs"], e, temps, rung, 1, 0, parity=kw["parity"], attempt=attempt, accept=accept)
    assert np.array_equal(temps, before[0]) and np.array_equal(rung, before[1])
    assert (attempt == 7).all() and (accept == 3).all()
    assert not tempering_ref.exchange_round(R // kw["n_rungs"], kw["n_rungs"], kw["parity"], 1, 0, 0, 0.0, e.tolist(),
                                            None, temps.tolist(), rung.tolist(), [0] * n_cnt, [0] * n_cnt)


def test_detailed_balance_on_harmonic_degrees_of_freedom():
    """20000 ladders of 6 rungs, geometric 200 ... 500 K, every replica's energy drawn from the exact
    canonical law of 20 harmonic degrees of freedom at the temperature it holds: Gamma(shape 20,
    scale T).  Exchanges that satisfy detailed balance leave that law alone, so after one even and
    one odd round the energies regrouped by rung still have mean 20 T_k and second moment 420 T_k^2.
    Bounds, derived and not tuned: 5 sigma of a mean over 20000 independent ladders,
      sigma(E)   = T_k sqrt(20 / 20000)                    (variance of Gamma: shape * scale^2)
      sigma(E^2) = T_k^2 sqrt(36120 / 20000)               (20*21*22*23 - 420^2 = 36120)
    The restatement with the sign of D flipped must break the bound: the check has power."""
    n_ladders, n_rungs, dof, seed = 20000, 6, 20, 777
    R = n_ladders * n_rungs
    ladder = moves.geometric_ladder(200.0, 500.0, n_rungs)
    temps0, rung0 = np.tile(ladder, n_ladders), moves.initial_rungs(R, n_rungs)
    e = np.random.default_rng(2024).gamma(dof, temps0)

    def deviations(rung):
        g = obs.by_rung(e, rung, n_rungs)                              # [n_rungs, n_ladders]
        d1 = np.abs(g.mean(1) - dof * ladder) / (ladder * np.sqrt(dof / n_ladders))
        d2 = np.abs((g * g).mean(1) - 420.0 * ladder ** 2) / (ladder ** 2 * np.sqrt(36120.0 / n_ladders))
        return d1, d2

    d1, d2 = deviations(rung0)
    assert (d1 < 5).all() and (d2 < 5).all(), (d1, d2)                 # the sample itself
    temps, rung = temps0.copy(), rung0.copy()
    attempt, accept = np.zeros(5, np.int64), np.zeros(5, np.int64)
    for rnd in (0, 1):
        exchange_round(n_rungs, e, temps, rung, seed, rnd, attempt=attempt, accept=accept)
    assert attempt.tolist() == [n_ladders] * 5
    assert 0.2 < accept.sum() / attempt.sum() < 0.95, accept / attempt
    assert np.array_equal(temps, ladder[rung])                         # the temperature a replica holds is its rung's
    d1, d2 = deviations(rung)
    print("deviations / sigma after the exchanges:", d1, d2, "acceptance", accept / attempt)
    assert (d1 < 5).all() and (d2 < 5).all(), (d1, d2)
    # power: the same two rounds with -D
    t_bad, r_bad = temps0.tolist(), rung0.tolist()
    for rnd in (0, 1):
        assert tempering_ref.exchange_round(n_ladders, n_rungs, rnd, seed, 0, rnd, 0.0, e.tolist(), None, t_bad, r_bad,
                                            [0] * 5, [0] * 5, sign=-1.0)
    b1, b2 = deviations(np.array(r_bad))
    assert (b1 > 5).any() and (b2 > 5).any(), (b1, b2)


def test_by_rung_on_a_hand_made_permutation():
    rung = np.array([2, 0, 1, 1, 2, 0], dtype=np.int32)               # two ladders of three
    v = np.arange(6) * 10.0
    assert obs.by_rung(v, rung, 3).tolist() == [[10.0, 50.0], [20.0, 30.0], [0.0, 40.0]]
    hist = np.arange(6 * 4).reshape(6, 4)                              # a [R, bins] per-replica result
    g = obs.by_rung(hist, rung, 3)
    assert g.shape == (3, 2, 4) and np.array_equal(g[0, 1], hist[5]) and np.array_equal(g[2, 0], hist[0])
    with pytest.raises(ValueError):
        obs.by_rung(v, np.array([0, 0, 1, 1, 2, 0]), 3)
    with pytest.raises(ValueError):
        obs.by_rung(v[:5], rung, 3)


def test_round_trips_on_hand_made_histories():
    #             replica 0: two journeys; 1: starts on top, one journey; 2: never reaches the top
    h = np.array([[0, 2, 1], [1, 1, 0], [2, 0, 1], [1, 1, 0], [0, 2, 1], [1, 1, 0], [2, 0, 1], [0, 1, 0]])
    assert obs.round_trips(h, n_rungs=3).tolist() == [2, 1, 0]
    assert obs.round_trips(h).tolist() == [2, 1, 0]
    assert obs.round_trips(h[:4], n_rungs=3).tolist() == [0, 0, 0]     # up and half-way down is no journey
    assert obs.round_trips(np.zeros((5, 2), dtype=int), n_rungs=3).tolist() == [0, 0]
    # top -> bottom -> top is not a journey; it counts only from the bottom
    assert obs.round_trips(np.array([[2], [1], [0], [1], [2]]), n_rungs=3).tolist() == [0]


def test_ladder_helpers():
    t = moves.geometric_ladder(260.0, 400.0, 16)
    assert t[0] == 260.0 and t[-1] == 400.0 and np.allclose(t[1:] / t[:-1], (400.0 / 260.0) ** (1 / 15), rtol=1e-14)
    assert moves.initial_rungs(12, 4).tolist() == [0, 1, 2, 3] * 3 and moves.initial_rungs(12, 4).dtype == np.int32
    for bad in ((12, 5), (4, 1), (3, 4)):
        with pytest.raises(ValueError):
            moves.initial_rungs(*bad)
    with pytest.raises(ValueError):
        moves.geometric_ladder(300.0, 300.0, 4)
    r = obs.exchange_acceptance([10, 0, 4], [5, 0, 4])
    assert r[0] == 0.5 and np.isnan(r[1]) and r[2] == 1.0


def test_shards_hold_whole_ladders():
    assert list(sharding.shard(24, 2, n_rungs=12)) == list(range(48, 72))
    assert list(sharding.shard_total(48, 1, 2, n_rungs=12)) == list(range(24, 48))
    assert list(sharding.shard(10, 1)) == list(range(10, 20))           # no ladder: as before
    with pytest.raises(ValueError, match="whole ladders"):
        sharding.shard(10, 1, n_rungs=4)
    with pytest.raises(ValueError, match="whole ladders"):
        sharding.shard_total(36, 0, 2, n_rungs=12)                      # 18 + 18
