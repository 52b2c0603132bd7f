"""Independent NPT replicas in one batch: a box per replica (mmc_batch_set_boxes and the per-box
volume move and chain).  Every replica is checked against the oracle at its own box and
kappa = alpha / L (Ewald/main.jl:290-291); the chains are replayed by the oracle step by step as
test_gpu_npt.test_npt_chain_on_the_batch_stepped_by_the_oracle does for one replica, and compared
with one-replica batches run through mmc_batch_run_npt."""
import math

import numpy as np
import pytest

import common
from common import rel

pytestmark = pytest.mark.gpu
TOL = 1e-9
RCUT = 10.0
ALPHA = 5.6
T, DR, DPHI = 298.15, 0.316555789, 0.05


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def host_rescale(a, L_new):
    """volumeChange.jl:62-80: COMs scale by f, atoms translate with their molecule."""
    f = L_new / a["box"]
    com = a["com"] * f
    d = com - a["com"]
    coords = a["coords"] + np.repeat(d, 3, axis=0)
    return dict(a, com=com, coords=coords, box=float(L_new))


def per_box_batch(states, rcut=RCUT):
    """A batch whose replica r holds states[r] (its own box); S(k) built."""
    from metropolismontecarlo_amd import structs
    from metropolismontecarlo_amd.device import Batch
    a0 = states[0]
    b = Batch(len(states), a0["com"], a0["coords"], a0["atype"], a0["charge"], a0["eps"], a0["sig"],
              a0["box"], ALPHA / a0["box"], structs.factor, rcut, rcut)
    for r, a in enumerate(states):
        b.set_replica(r, a["com"], a["coords"])
    b.set_boxes([a["box"] for a in states], ALPHA)
    b.recip_long()
    return b


def oracle_totals(orc, a, rcut=RCUT):
    L = a["box"]
    return orc.potential_ewald(common.oracle_system(a), orc.Ewald(ALPHA / L, 5, 27, L), rcut, rcut)


def nist4_boxes(factors):
    a = common.nist_arrays(4, "unwrapped")
    return [host_rescale(a, a["box"] * f) for f in factors]


def test_totals_at_eight_boxes(orc):
    """Each replica's potential() at its own box and alpha / L equals the oracle's."""
    states = nist4_boxes(np.linspace(0.94, 1.06, 8))
    with per_box_batch(states) as b:
        assert np.array_equal(b.get_boxes(), [a["box"] for a in states])
        t = b.potential_ewald(as_array=True)
        for r, a in enumerate(states):
            to = oracle_totals(orc, a)
            for key in ("energy", "virial", "lj", "real", "recip", "self"):
                assert rel(t[key][r], to[key], 1.0) < TOL, (r, key)
        # RecipLong alone, per box (no factor)
        e = b.recip_long()
        for r, a in enumerate(states):
            assert rel(e[r] * b.factor, oracle_totals(orc, a)["recip"]) < TOL, r


def test_batched_volume_move_restores_rejected_and_matches_the_oracle(orc):
    """One batched trial over 8 replicas (some not moving), a mixed settle: rejected and unmoved
    replicas give back coordinates, S(k), box and totals bit for bit, accepted ones equal the
    oracle, and trial moves afterwards agree with a twin batch that never tried the move."""
    states = nist4_boxes(np.linspace(0.95, 1.05, 8))
    R = len(states)
    boxes = np.array([a["box"] for a in states])
    new = boxes * np.array([1.01, 0.0, 0.985, 1.02, 0.0, 0.99, 1.004, 0.97])
    accept = np.array([1, 1, 0, 1, 0, 0, 1, 1], dtype=np.int32)   # (replicas 1, 4 do not move)
    kept = [r for r in range(R) if not (new[r] != 0 and accept[r])]
    with per_box_batch(states) as b:
        t0 = b.potential_ewald(as_array=True).copy()
        before = [b.get_replica(r) for r in range(R)]
        tot = b.volume_trial_replicas(new)
        for r in range(R):
            if new[r] == 0:
                assert all(tot[k][r] == t0[k][r] for k in ("energy", "lj", "real", "recip", "self"))
                continue
            to = oracle_totals(orc, host_rescale(states[r], new[r]))
            for key in ("energy", "lj", "real", "recip", "self"):
                assert rel(tot[key][r], to[key], 1.0) < TOL, (r, key)
        b.volume_settle(accept)
        after_boxes = b.get_boxes()
        t1 = b.potential_ewald(as_array=True).copy()
        for r in kept:
            after = b.get_replica(r)
            assert all(np.array_equal(x, y) for x, y in zip(before[r], after)), r
            assert after_boxes[r] == boxes[r]
            assert all(t1[k][r] == t0[k][r] for k in ("energy", "lj", "real", "recip", "self")), r
        final = []
        for r in range(R):
            com, coords, _ = b.get_replica(r)
            if r in kept:
                final.append(states[r])
                continue
            a2 = host_rescale(states[r], new[r])
            assert after_boxes[r] == new[r]
            assert np.array_equal(com, a2["com"]) and np.array_equal(coords, a2["coords"]), r
            assert rel(t1["energy"][r], oracle_totals(orc, a2)["energy"]) < TOL, r
            final.append(a2)
        # the chains go on exactly like those of a batch that never tried the move
        with per_box_batch(final) as twin:
            t2 = twin.potential_ewald(as_array=True)
            assert np.array_equal(t2["energy"], t1["energy"])
            e1, st = b.run(60, T, DR, DPHI, seed=77, energies=t1["energy"].copy())
            e2, _ = twin.run(60, T, DR, DPHI, seed=77, energies=t2["energy"].copy())
            assert st["moves"] == 60 * R and st["server_steps"] == 0
            assert np.array_equal(e1, e2)
            for r in range(R):
                assert all(np.array_equal(x, y) for x, y in zip(b.get_replica(r), twin.get_replica(r))), r
            t3 = b.potential_ewald(as_array=True)
            assert np.abs(e1 - t3["energy"]).max() < TOL * np.abs(t3["energy"]).max()


# ---- the chains ----------------------------------------------------------------------------------
CHAIN = dict(seed=424242, rep0=3, n_sweeps=5, per_sweep=40, factors=(0.97, 1.0, 1.02, 1.045),
             pressures=(0.0, 0.02, 0.05, 0.1), vmax_frac=0.02)


def chain_states():
    return nist4_boxes(CHAIN["factors"])


def oracle_npt_chain(orc, a, replica, pressure, vmax, seed, n_sweeps, per_sweep, rc=RCUT,
                     lj_rc=None, log=None):
    """mmc_batch_run_npt's rule for one chain, on the oracle: proposals rebuilt from the Philox
    draws of (seed, replica), dU from orc.trial_move, the volume move's uniforms from slot
    MMC_SLOT_VOLUME, its energy from orc.potential_ewald on coordinates rescaled on the host
    (volumeChange.jl:59-147).  rc is the Coulomb cutoff, lj_rc the LJ one (default rc).  `log`, a
    list, gets each sweep's volume move: "refused" (box below 2 r_cut), "accepted" or "rejected".
    Returns (box, com, coords, energy, trial accepts, volume accepts)."""
    lj_rc = rc if lj_rc is None else lj_rc
    from test_gpu_batch import _rigid_proposal
    from test_gpu_moves import philox_pair
    n_mol = a["com"].shape[0]
    cur = dict(a)
    s = common.oracle_system(cur)
    box = a["box"]
    ew = orc.Ewald(ALPHA / box, 5, 27, box)
    energy = orc.potential_ewald(s, ew, lj_rc, rc)["energy"]
    step, n_acc, n_acc_vol = 0, 0, 0
    for sweep in range(n_sweeps):
        for k in range(per_sweep):
            i = k % n_mol                                   # every run restarts its sweep (main.jl:490)
            kind, c_new, a_new, u = _rigid_proposal(seed, replica, step, s.com[i].copy(),
                                                    s.coords[3 * i:3 * i + 3].copy(), box, DR, DPHI)
            d, ov = orc.trial_move(i + 1, s, ew, lj_rc, rc, c_new, a_new)
            delta = d[0] + d[1] + d[2]
            x = delta / T
            if (x < 0.0 or math.exp(-x) > u) and not ov:
                energy += delta
                s.com[i] = c_new
                s.coords[3 * i:3 * i + 3] = a_new
                ew.sumQExpOld = ew.sumQExpNew.copy()
                n_acc += 1
            else:
                ew.sumQExpNew = ew.sumQExpOld.copy()
            step += 1
        ua, ub = philox_pair(seed, replica, step, 0x40000000)  # MMC_SLOT_VOLUME
        vol_old = box ** 3
        vol_new = vol_old + (ua - 0.5) * vmax                   # volumeChange.jl:59
        L_new = vol_new ** (1.0 / 3.0)
        if max(rc, lj_rc) > L_new / 2:
            if log is not None:
                log.append("refused")
            continue
        a2 = host_rescale(dict(cur, com=s.com.copy(), coords=s.coords.copy(), box=box), L_new)
        s2 = common.oracle_system(a2)
        ew2 = orc.Ewald(ALPHA / L_new, 5, 27, L_new)
        e_new = orc.potential_ewald(s2, ew2, lj_rc, rc)["energy"]
        arg = -(1.0 / T) * (pressure * (vol_new - vol_old) - n_mol * math.log(vol_new / vol_old) * T
                            + (e_new - energy))                 # :129-130
        if ub < math.exp(min(arg, 700.0)):                      # :132
            s, ew, box, energy, cur = s2, ew2, L_new, e_new, a2
            n_acc_vol += 1
            if log is not None:
                log.append("accepted")
        elif log is not None:
            log.append("rejected")
    return box, s.com, s.coords, energy, n_acc, n_acc_vol


@pytest.fixture(scope="module")
def per_box_chains():
    """run_npt_replicas on 4 replicas of NIST configuration 4 at different boxes and pressures."""
    states = chain_states()
    vmax = CHAIN["vmax_frac"] * states[0]["box"] ** 3
    with per_box_batch(states) as b:
        e0 = b.potential_ewald(as_array=True)["energy"].copy()
        e1, st, ns = b.run_npt_replicas(CHAIN["n_sweeps"], T, 0.0, vmax, DR, DPHI, CHAIN["seed"], e0,
                                        moves_per_sweep=CHAIN["per_sweep"], alpha=ALPHA,
                                        pressures=CHAIN["pressures"], replica0=CHAIN["rep0"])
        reps = [b.get_replica(r) for r in range(len(states))]
        boxes = b.get_boxes()
        t_end = b.potential_ewald(as_array=True).copy()
    return dict(states=states, vmax=vmax, e0=e0, e1=e1, st=st, ns=ns, reps=reps, boxes=boxes,
                t_end=t_end)


def test_npt_replicas_stepped_by_the_oracle(per_box_chains, orc):
    c = per_box_chains
    R = len(c["states"])
    assert c["st"]["moves"] == R * CHAIN["n_sweeps"] * CHAIN["per_sweep"]
    n_acc_total, vol_acc = 0, []
    for r in range(R):
        box, com, coords, energy, n_acc, n_acc_vol = oracle_npt_chain(
            orc, c["states"][r], CHAIN["rep0"] + r, CHAIN["pressures"][r], c["vmax"], CHAIN["seed"],
            CHAIN["n_sweeps"], CHAIN["per_sweep"])
        ns = c["ns"][r]
        assert ns["vol_attempt"] == CHAIN["n_sweeps"]
        assert ns["vol_accept"] == n_acc_vol, r
        assert ns["box"] == pytest.approx(box, rel=1e-15) and c["boxes"][r] == ns["box"]
        gcom, gcoords, _ = c["reps"][r]
        assert np.abs(gcom - com).max() < 1e-11 and np.abs(gcoords - coords).max() < 1e-11, r
        assert abs(c["e1"][r] - energy) < TOL * abs(energy), r
        assert rel(c["t_end"]["energy"][r], energy) < TOL, r
        n_acc_total += n_acc
        vol_acc.append(n_acc_vol)
    assert c["st"]["trans_accept"] + c["st"]["rot_accept"] == n_acc_total
    assert 0 < sum(vol_acc) < R * CHAIN["n_sweeps"], "parameters must accept some volume moves and reject some"


def test_npt_replicas_equal_one_replica_batches(per_box_chains):
    """Replica r of the per-box batch against a one-replica batch with replica0 = rep0 + r run by
    mmc_batch_run_npt: the same decisions, box and energies (different kernels: not bit for bit)."""
    from test_gpu_npt import make_one_replica_batch
    c = per_box_chains
    for r, a in enumerate(c["states"]):
        with make_one_replica_batch(a) as b1:
            e0 = float(b1.potential_ewald(as_array=True)["energy"][0])
            assert rel(e0, c["e0"][r]) < 1e-12
            e1, st, ns = b1.run_npt(CHAIN["n_sweeps"], T, CHAIN["pressures"][r], c["vmax"], DR, DPHI,
                                    CHAIN["seed"], e0, moves_per_sweep=CHAIN["per_sweep"], alpha=ALPHA,
                                    replica0=CHAIN["rep0"] + r)
        assert ns["vol_accept"] == c["ns"][r]["vol_accept"] and ns["vol_attempt"] == c["ns"][r]["vol_attempt"]
        assert ns["box"] == c["ns"][r]["box"]
        assert rel(e1, c["e1"][r]) < 1e-12, r
        assert ns["volume_sum"] == pytest.approx(c["ns"][r]["volume_sum"], rel=1e-15)


# ---- guards --------------------------------------------------------------------------------------
def test_table_domain_is_checked_at_twice_the_cutoff():
    """NIST configuration 2 at r_cut 9: kappa * sqrt(r_cut^2 + 100) = 4.18 > 4 at L = 2 r_cut."""
    from metropolismontecarlo_amd._lib import MMCError
    a = common.nist_arrays(2, "unwrapped")
    with plain_batch(a, 3, 9.0) as b:
        t0 = b.potential_ewald(as_array=True).copy()
        before = b.get_replica(1)
        with pytest.raises(MMCError, match="MMC_ERR_UNSUPPORTED"):
            b.set_boxes([a["box"]] * 3, ALPHA)
        assert np.array_equal(b.get_boxes(), [a["box"]] * 3)
        with pytest.raises(MMCError, match="MMC_ERR_UNSUPPORTED"):
            b.run_npt_replicas(1, T, 0.0, 100.0, DR, DPHI, 1, t0["energy"])
        assert all(np.array_equal(x, y) for x, y in zip(before, b.get_replica(1)))
        t1 = b.potential_ewald(as_array=True)
        assert all(np.array_equal(t0[k], t1[k]) for k in ("energy", "lj", "real", "recip", "self"))
        # ... and the batch is as usable as before
        e, st = b.run(20, T, DR, DPHI, seed=3, energies=t1["energy"].copy())
        assert st["moves"] == 60


def plain_batch(a, R, rcut):
    from metropolismontecarlo_amd import structs
    from metropolismontecarlo_amd.device import Batch
    return Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
                 ALPHA / a["box"], structs.factor, rcut, rcut)


def test_one_box_entry_points_refuse_a_per_box_batch():
    from metropolismontecarlo_amd._lib import MMCError
    states = nist4_boxes((0.98, 1.02))
    with per_box_batch(states) as b:
        e = b.potential_ewald(as_array=True)["energy"].copy()
        L = states[0]["box"]
        calls = {
            "rdf": lambda: b.rdf(0, 50),
            "run_chains": lambda: b.run_chains(b.new_chains(e), 10, T, seed=1),
            "kernel 2": lambda: b.set_option("kernel", 2),
            "kernel 4": lambda: b.set_option("kernel", 4),
            "persistent": lambda: b.set_option("persistent", 1),
            "host moves": lambda: b.set_option("device_moves", 0),
            "volume_change": lambda: b.volume_change(L, ALPHA / L),
            "volume_trial": lambda: b.volume_trial(L, ALPHA / L),
            "volume_accept": lambda: b.volume_accept(),
            "volume_reject": lambda: b.volume_reject(),
            "run_npt": lambda: b.run_npt(1, T, 0.0, 100.0, DR, DPHI, 1, float(e[0])),
            "eval": lambda: b.eval([1, 1], states[0]["com"][:2], states[0]["coords"][:6].reshape(2, 3, 3)),
            "qq_table": lambda: b.qq_table([4.0]),
        }
        for name, call in calls.items():
            with pytest.raises(MMCError, match="MMC_ERR_UNSUPPORTED"):
                call()
        # nothing above changed the batch
        t = b.potential_ewald(as_array=True)
        assert np.array_equal(t["energy"], e)
        assert np.array_equal(b.get_boxes(), [a["box"] for a in states])
