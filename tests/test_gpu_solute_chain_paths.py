"""Chains around a fixed solute on every run path (include/mmc_hip.h, "A fixed solute"), stepped by the
oracle on the N + 1 molecule system: mmc_batch_run with device and host proposals, one and three
parts, candidate lists on and off, mmc_batch_run_chains and mmc_batch_run_exchange; the null solute
and the removed solute bit for bit; every fence; save and load.

Shapes: 65 waters (the first 65 of NIST config 3, 20 A), R = 3 (4 for the ladder), two sweeps = 130
steps.  A device-made chain is replayed step by step (solute_chain_ref.replay: the proposal rebuilt
from the exported Philox draws, dU from the oracle's trial move of the N + 1 system, Metropolis with
the step's own uniform) against option "trace_steps"; a chain of host proposals likewise, its draws
the driver's own xoshiro256++ restated in solute_chain_ref.HostRng.  Tolerances: TOL (|dU| + 1e4) per
step as test_gpu_replay_paths.py; 1e-9 on S(k); the running energy within 1e-9 of the size of a fresh
total (the project's bound: test_gpu_batch.py, test_gpu_moves.py).  Final coordinates: 2e-13 A, not
bitwise -- the replay rebuilds every proposal in Python (numpy products and math.sin / cos where the
device and the driver have their own sine, cosine and fused products), so an accepted rotation may
differ from the batch's in the last bit, and the differences add up along 130 steps; decisions and
flags are compared exactly."""
import numpy as np
import pytest

import common
import solute_chain_ref as scr
import solute_ref as sr
from metropolismontecarlo_amd import _lib
from metropolismontecarlo_amd import structs

pytestmark = pytest.mark.gpu

LJ, QQ, T, DR, DPHI = 8.5, 9.5, sr.T, 0.3, 0.25
N, STEPS, TOL = 65, 130, 1e-9


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def water():
    return sr.first_molecules(common.nist_arrays(3, "unwrapped"), N)


def make_batch(a, R, lj=LJ, qq=QQ, alpha=5.6):
    from metropolismontecarlo_amd.device import Batch
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
              alpha / a["box"], structs.factor, lj, qq)
    b.recip_long()
    return b


def placed_in_the_water(a, sol):
    """The solute's reference point 2.6 A from the centre of mass of the water nearest to the box's
    corner, through the corner: inside the first shell of several waters, images on all three axes.
    The first orientation (seeds 1, 2, ...) that keeps every site 1.2 A from every water atom: the
    chain starts from a finite energy."""
    box = float(a["box"])
    d = np.minimum(a["com"], box - a["com"])
    j = int(np.argmin((d * d).sum(1)))
    c = (a["com"][j] + 2.6 * sr.GATE_DIRS[2]) % box
    for seed in range(1, 200):
        mol = sr.placed(sol.offsets, c, sr.rotation(np.random.default_rng(seed)))
        dd = mol[:-1, None, :] - np.asarray(a["coords"])[None, :, :]
        dd = dd + common.image_shift(dd, box)
        if (dd * dd).sum(2).min() > 1.2 ** 2:
            return mol
    raise AssertionError("no orientation of the solute fits")


def solute_of(name, a):
    return {"methane": sr.methane, "cation": sr.cation, "dipole": sr.dipole,
            "synthetic16": lambda a: sr.synthetic(a, 16, seed=7)}[name](a)


def proposal_of(seed, replica, box, dr=DR, dphi=DPHI):
    from test_gpu_batch import _rigid_proposal
    return lambda step, com, atoms: _rigid_proposal(seed, replica, step, com, atoms, box, dr, dphi)


def check_trace(trace, d_gpu, f_gpu, r, at):
    worst = 0.0
    for step, (delta, flags) in enumerate(trace):
        worst = max(worst, abs(d_gpu[r, step] - delta))
        assert abs(d_gpu[r, step] - delta) < TOL * (abs(delta) + 1e4), (at, r, step, d_gpu[r, step], delta)
        assert f_gpu[r, step] == flags, (at, r, step, f_gpu[r, step], flags)
    return worst


def check_final(final, n1, r, at):
    """What the chain left of replica r (get_replica before anything rebuilt S(k): the incrementally
    updated sums) against the oracle's chain `n1`: coordinates, and S(k) against the oracle's fresh
    RecipLong of the N + 1 system."""
    com, coords, S = final
    assert np.abs(com - n1.s.com[:-1]).max() < 2e-13 and np.abs(coords - n1.s.coords[:3 * N]).max() < 2e-13, (at, r)
    n1.recip_long()
    assert np.abs(S - n1.ew.sumQExpOld).max() < 1e-9, (at, r, np.abs(S - n1.ew.sumQExpOld).max())
    return com, coords


def check_kernel_and_lists(b, opts, n_parts, n_moves, at):
    """A row that names the wave kernel (option "kernel" = 2; batch_kernel_for then takes it whatever the
    size) shows by mmc_batch_cand_stats which scan its steps made.  The counters are the wave kernel's own,
    kept only where a launch has lists to count against (k_move_eval_wave: one part per move and a
    CandView): with the lists on and one part every step is counted once, on its list or on the full scan;
    with the lists off, or with several parts per move, no list is ever allocated and nothing is counted --
    the state word says which of the two it was (0: switched off; 4: never asked for, as the several-parts
    form marks the lists stale and does not prepare them)."""
    if opts.get("kernel") != 2:
        return
    c = b.cand_stats()
    print(f"  {at}: cand_stats {c}")
    if opts.get("candidate_lists", 1) and n_parts == 1:
        assert c["state"] == 1 and c["list_steps"] > 0 and c["list_steps"] + c["scan_steps"] == n_moves, (at, c)
    else:
        assert c["list_steps"] == 0 and c["scan_steps"] == 0 and c["bytes"] == 0, (at, c)
        assert c["state"] == (0 if n_parts == 1 else 4), (at, c)


# The rows of kernel 2 run k_move_eval_wave at R = 3, where the size alone (kernel 3) picks the
# workgroup-per-move kernel: ("cation", {"candidate_lists": 0}, 1) above them is therefore a row of kernel 1.
# At this box (20 A, gate 9.5 A) the image-by-molecule form does not apply (gate + 2 r_mol > L / 2), so the
# row with "image_by_molecule" = 0 runs the same form as the one without and holds the option's handling.
@pytest.mark.parametrize("name,opts,n_parts", [
    ("cation", {}, 1), ("cation", {"candidate_lists": 0}, 1), ("dipole", {}, 3), ("methane", {"kernel": 1}, 1),
    ("synthetic16", {"accept_on_device": 1, "steps_per_launch": 8}, 1), ("dipole", {"kernel": 0}, 3),
    ("cation", {"kernel": 2}, 1), ("dipole", {"kernel": 2, "candidate_lists": 0}, 1),
    ("synthetic16", {"kernel": 2, "image_by_molecule": 0}, 1), ("dipole", {"kernel": 2}, 3),
])
def test_device_made_chains_stepped_by_the_oracle(orc, water, name, opts, n_parts):
    a, R, seed = water, 3, 4321
    sol, box = solute_of(name, a), float(a["box"])
    mol = placed_in_the_water(a, sol)
    so = sr.SoluteOracle(orc, a, sol, LJ, QQ)
    with make_batch(a, R) as b:
        b.set_option("device_moves", 1)
        for k, v in opts.items():
            b.set_option(k, v)
        b.set_solute(sol, mol)
        e0 = b.potential_ewald(as_array=True)["energy"].copy()
        b.set_option("trace_steps", STEPS)
        e1, st = b.run(STEPS, T, DR, DPHI, seed=seed, energies=e0, n_parts=n_parts, n_threads=2)
        d_gpu, f_gpu = b.get_trace(STEPS)
        finals = [b.get_replica(r) for r in range(R)]
        assert st["moves"] == R * STEPS and st["device_decisions"] == 0 and st["server_steps"] == 0
        check_kernel_and_lists(b, opts, n_parts, R * STEPS, (name, opts, n_parts))
        fresh = b.potential_ewald(as_array=True)
        assert np.abs(e1 - fresh["energy"]).max() < 1e-9 * np.abs(fresh["energy"]).max(), (e1, fresh["energy"])
        worst = 0.0
        for r in range(R):
            n1 = scr.N1(so, a["com"], a["coords"], mol, box)
            trace, e_acc, _ = scr.replay(n1, proposal_of(seed, r, box), STEPS, T)
            worst = max(worst, check_trace(trace, d_gpu, f_gpu, r, (name, opts)))
            assert abs((e1[r] - e0[r]) - e_acc) < TOL * 1e5, (name, r)
            check_final(finals[r], n1, r, (name, opts))
            to = n1.potential()
            for key in ("energy", "lj", "real", "recip"):
                assert common.rel(fresh[key][r], to[key]) < TOL, (name, r, key, fresh[key][r], to[key])
            assert sum(f & 1 for _, f in trace) > 10          # the chain moves
    print(f"chain {name} {opts} parts={n_parts}: largest |dU - oracle| over {R * STEPS} steps {worst:.3e}")


@pytest.mark.parametrize("name,n_parts,opts", [("cation", 1, {}), ("dipole", 3, {}), ("synthetic16", 1, {"zero_copy_moves": 1}),
                                               ("dipole", 1, {"kernel": 2})])
def test_chains_of_host_proposals_stepped_by_the_oracle(orc, water, name, n_parts, opts):
    """The driver proposes on the host: k_solute_move reads the step's records from the host-proposal
    buffer (copied to the device, or with zero_copy_moves in place) instead of a ring slot.  The
    chain's draws are the driver's own generator, restated in solute_chain_ref.HostRng /
    host_proposal; every step's dU and decision, the final coordinates and S(k) as for the
    device-made chains."""
    a, R, seed = water, 3, 99
    sol, box = solute_of(name, a), float(a["box"])
    mol = placed_in_the_water(a, sol)
    so = sr.SoluteOracle(orc, a, sol, LJ, QQ)
    with make_batch(a, R) as b:
        for k, v in opts.items():
            b.set_option(k, v)
        b.set_solute(sol, mol)
        e0 = b.potential_ewald(as_array=True)["energy"].copy()
        b.set_option("trace_steps", STEPS)
        e1, st = b.run(STEPS, T, DR, DPHI, seed=seed, energies=e0, n_parts=n_parts, n_threads=2)
        d_gpu, f_gpu = b.get_trace(STEPS)
        finals = [b.get_replica(r) for r in range(R)]
        assert st["moves"] == R * STEPS and st["device_decisions"] == 0 and st["server_steps"] == 0
        check_kernel_and_lists(b, opts, n_parts, R * STEPS, (name, "host", opts, n_parts))
        fresh = b.potential_ewald(as_array=True)
        assert np.abs(e1 - fresh["energy"]).max() < 1e-9 * np.abs(fresh["energy"]).max(), (e1, fresh["energy"])
        worst = 0.0
        for r in range(R):
            n1 = scr.N1(so, a["com"], a["coords"], mol, box)
            trace, e_acc, _ = scr.replay(n1, scr.host_proposal(scr.HostRng(seed, r), box, DR, DPHI), STEPS, T)
            worst = max(worst, check_trace(trace, d_gpu, f_gpu, r, (name, "host")))
            assert abs((e1[r] - e0[r]) - e_acc) < TOL * 1e5, (name, r)
            check_final(finals[r], n1, r, (name, "host"))
            to = n1.potential()
            for key in ("energy", "lj", "real", "recip"):
                assert common.rel(fresh[key][r], to[key]) < TOL, (name, r, key, fresh[key][r], to[key])
            assert sum(f & 1 for _, f in trace) > 10 and 10 < sum(f >> 2 & 1 for _, f in trace) < STEPS - 10
    print(f"chain {name} host proposals parts={n_parts} {opts}: largest |dU - oracle| over {R * STEPS} steps {worst:.3e}")


def test_run_chains_with_the_solutes_virial(orc, water):
    a, R, seed = water, 3, 777
    sol, box = sr.dipole(a), float(a["box"])
    mol = placed_in_the_water(a, sol)
    so = sr.SoluteOracle(orc, a, sol, LJ, QQ)
    with make_batch(a, R) as b:
        b.set_option("device_moves", 1)
        b.set_solute(sol, mol)
        t0 = b.potential_ewald(as_array=True).copy()
        chains = b.new_chains(t0["energy"], t0["virial"], dr_max=DR, dphi_max=DPHI)
        b.set_option("trace_steps", STEPS)
        st = b.run_chains(chains, STEPS, T, seed=seed, adjust=False, n_threads=2)
        d_gpu, f_gpu = b.get_trace(STEPS)
        finals = [b.get_replica(r) for r in range(R)]
        assert st["device_decisions"] == 0
        t1 = b.potential_ewald(as_array=True)
        for r in range(R):
            n1 = scr.N1(so, a["com"], a["coords"], mol, box)
            trace, e_acc, v_acc = scr.replay(n1, proposal_of(seed, r, box), STEPS, T)
            check_trace(trace, d_gpu, f_gpu, r, "run_chains")
            check_final(finals[r], n1, r, "run_chains")
            assert abs((chains["energy"][r] - t0["energy"][r]) - e_acc) < TOL * 1e5
            assert abs((chains["virial"][r] - t0["virial"][r]) - v_acc) < TOL * 1e5, (chains["virial"][r], v_acc)
            # the running virial is the fresh total's: the solute's pairs are in both
            assert abs(chains["virial"][r] - t1["virial"][r]) < 1e-9 * abs(t1["virial"][r])
            assert abs(chains["energy"][r] - t1["energy"][r]) < 1e-9 * abs(t1["energy"][r])
            assert chains["steps_taken"][r] == STEPS


def test_run_exchange_with_per_replica_temperatures(orc, water):
    a, R, seed = water, 4, 31
    sol, box = sr.cation(a), float(a["box"])
    mol = placed_in_the_water(a, sol)
    so = sr.SoluteOracle(orc, a, sol, LJ, QQ)
    temps = np.array([280.0, 300.0, 325.0, 355.0])
    with make_batch(a, R) as b:
        b.set_option("device_moves", 1)
        b.set_solute(sol, mol)
        b.set_temperatures(temps)
        e0 = b.potential_ewald(as_array=True)["energy"].copy()
        rung = np.arange(4, dtype=np.int32)
        b.set_option("trace_steps", STEPS)
        e1, st, attempt, accept = b.run_exchange(1, STEPS, DR, DPHI, seed, e0, rung, 4, n_threads=2)
        d_gpu, f_gpu = b.get_trace(STEPS)
        finals = [b.get_replica(r) for r in range(R)]
        assert st["device_decisions"] == 0 and attempt.sum() >= 1
        fresh = b.potential_ewald(as_array=True)["energy"]
        assert np.abs(e1 - fresh).max() < 1e-9 * np.abs(fresh).max()
        for r in range(R):
            n1 = scr.N1(so, a["com"], a["coords"], mol, box)
            trace, e_acc, _ = scr.replay(n1, proposal_of(seed, r, box), STEPS, temps[r])
            check_trace(trace, d_gpu, f_gpu, r, "run_exchange")
            check_final(finals[r], n1, r, "run_exchange")
            assert abs((e1[r] - e0[r]) - e_acc) < TOL * 1e5
        assert sorted(b.temperatures()) == sorted(temps)      # the exchange permutes the ladder, no more


# ---- the null solute, and a solute taken away ---------------------------------------------------------
def chain_state(b, seed, n_parts=1, opts=None):
    """Run STEPS steps and return everything a chain leaves: trace, energies, state records."""
    for k, v in (opts or {}).items():
        b.set_option(k, v)
    e0 = b.potential_ewald(as_array=True)["energy"].copy()
    b.set_option("trace_steps", STEPS)
    e1, st = b.run(STEPS, T, DR, DPHI, seed=seed, energies=e0, n_parts=n_parts, n_threads=2)
    d, f = b.get_trace(STEPS)
    return dict(e0=e0.tobytes(), e1=e1.tobytes(), d=d.tobytes(), f=f.tobytes(), rec=b.get_state().tobytes()), st


@pytest.mark.parametrize("device_moves,n_parts,kernel", [
    pytest.param(1, 1, 3, id="1-1"), pytest.param(1, 3, 3, id="1-3"), pytest.param(0, 1, 3, id="0-1"),   # (3: by size, the default)
    pytest.param(1, 1, 2, id="1-1-wave")])
def test_a_null_solute_changes_no_bit(water, device_moves, n_parts, kernel):
    a = water
    null = structs.Solute("null", [[0.0, 0.0, 0.0], [0.7, 0.1, 0.0]], [0.0, 0.0], np.zeros((2, 3)), np.zeros((2, 3)))
    out = []
    for with_solute in (False, True):
        with make_batch(a, 3) as b:
            b.set_option("device_moves", device_moves)
            if with_solute:
                b.set_solute(null, placed_in_the_water(a, null))
            # (the path a solute takes: the host decides, a launch per step -- not the move server)
            out.append(chain_state(b, 55, n_parts, {"accept_on_device": 0, "persistent": 0, "kernel": kernel})[0])
            if kernel == 2:      # the wave kernel on its candidate lists, with the solute's record and without
                c = b.cand_stats()
                assert c["state"] == 1 and c["list_steps"] > 0 and c["list_steps"] + c["scan_steps"] == 3 * STEPS, c
    for k in out[0]:
        assert out[0][k] == out[1][k] or k == "rec", k
    # the state records differ in nothing either: the info carries the solute, the records do not
    assert out[0]["rec"] == out[1]["rec"]


def test_a_removed_charged_solute_leaves_the_plain_batch(water):
    a = water
    sol = sr.dipole(a)
    out = []
    for had_solute in (False, True):
        with make_batch(a, 3) as b:
            b.set_option("device_moves", 1)
            if had_solute:
                b.set_solute(sol, placed_in_the_water(a, sol))
                b.recip_long()
                assert b.get_replica(0)[2].tobytes() != make_s0(a)
                b.set_solute(None)
                b.recip_long()
            out.append(chain_state(b, 56)[0])
    assert out[0] == out[1]


def make_s0(a):
    with make_batch(a, 1) as b:
        return b.get_replica(0)[2].tobytes()


# ---- fences -------------------------------------------------------------------------------------------
def test_everything_whose_energies_would_be_another_systems_is_refused(water):
    a = water
    sol, box = sr.dipole(a), float(a["box"])
    mol = placed_in_the_water(a, sol)
    pair = structs.SolutePair(sr.methane(a), sr.cation(a), [[100.0]], [[3.0]])
    with make_batch(a, 3) as b:
        b.set_option("device_moves", 1)
        b.set_solute(sol, mol)
        b.recip_long()
        rec, info = b.get_state().tobytes(), bytes(b.state_info())
        e = np.zeros(3)
        calls = {
            "set_boxes": lambda: b.set_boxes(np.full(3, box)),
            "wolf": lambda: b.set_coulomb_style("wolf"),
            "potential_wolf": lambda: b.potential_wolf(),
            "volume_change": lambda: b.volume_change(box * 1.01, 5.6 / (box * 1.01)),
            "volume_trial": lambda: b.volume_trial(box * 1.01, 5.6 / (box * 1.01)),
            "volume_accept": lambda: b.volume_accept(),
            "volume_reject": lambda: b.volume_reject(),
            "run_npt": lambda: b.run_npt(1, T, 1.0, 10.0, DR, DPHI, 3, 0.0),
            "widom": lambda: b.widom(2, T, seed=1),
            "widom_at": lambda: b.widom_at(np.ones((3, 1, 12)), T),
            "widom_solute": lambda: b.widom_solute(sol, 2, T, seed=1),
            "widom_solute_at": lambda: b.widom_solute_at(sol, np.ones((3, 1, 3, 3)), T),
            "widom_pair": lambda: b.widom_pair(pair, [4.0], 2, T, seed=1),
            "widom_pair_at": lambda: b.widom_pair_at(pair, np.ones((3, 1, 2, 3)), np.ones((3, 1, 1, 2, 3)), T),
            "deletion": lambda: b.deletion(T),
            "forces": lambda: b.forces(),
            "volume_perturb": lambda: b.volume_perturb(T, scales=[1.001]),
            "pair_energy": lambda: b.pair_energy(10),
        }
        for name, call in calls.items():
            with pytest.raises(_lib.MMCError, match="MMC_ERR_UNSUPPORTED") as ei:
                call()
            assert "solute" in str(ei.value), (name, str(ei.value))
            assert b.get_state().tobytes() == rec and bytes(b.state_info()) == info, name
        # the run paths that have no launch per step, asked for by name
        for key, value in (("persistent", 1), ("kernel", 4)):
            b.set_option(key, value)
            with pytest.raises(_lib.MMCError, match="MMC_ERR_UNSUPPORTED.*solute"):
                b.run(10, T, DR, DPHI, seed=1, energies=e)
            if key == "kernel":      # ... and from mmc_batch_eval, which has the same kernels
                with pytest.raises(_lib.MMCError, match="MMC_ERR_UNSUPPORTED.*solute"):
                    b.eval(1, np.tile(a["com"][0], (3, 1)), np.tile(a["coords"][:3], (3, 1, 1)))
            b.set_option(key, -1 if key == "persistent" else 3)
            assert b.get_state().tobytes() == rec
        # the observables that read coordinates only stay open
        b.rdf_sites(10)
        b.dipoles()
        b.local_order()
        # ... and with the solute gone everything is open again
        b.set_solute(None)
        b.recip_long()
        b.widom(2, T, seed=1)
        b.forces()


def test_a_solute_is_refused_where_the_batch_cannot_take_it(water):
    a = water
    sol, box = sr.dipole(a), float(a["box"])
    mol = placed_in_the_water(a, sol)

    def refused(b):
        rec = b.get_state().tobytes()
        with pytest.raises(_lib.MMCError, match="MMC_ERR_UNSUPPORTED"):
            b.set_solute(sol, mol)
        assert b.get_solute() is None and b.get_state().tobytes() == rec and not b.state_info().solute_on
    with make_batch(a, 2, lj=10.0, qq=10.0) as b:   # (kappa = alpha / (2 r_cut) inside the erfc table)
        b.set_option("device_moves", 1)
        b.set_boxes(np.full(2, box))
        b.recip_long()
        refused(b)
    with make_batch(a, 2) as b:
        b.set_coulomb_style("wolf")
        refused(b)
    with make_batch(a, 2, alpha=7.0) as b:           # kappa sqrt(r_cut^2 + 100) = 4.8: beyond the erfc table
        refused(b)
    with make_batch(a, 2) as b:                      # outstanding proposals: a matter of state
        b.eval(1, np.tile(a["com"][0], (2, 1)), np.tile(a["coords"][:3], (2, 1, 1)))
        with pytest.raises(_lib.MMCError, match="MMC_ERR_STATE"):
            b.set_solute(sol, mol)
        b.settle(np.zeros(2, dtype=np.int32))
        b.set_solute(sol, mol)
        assert b.state_info().solute_on and b.state_info().solute_hash == scr.solute_hash(sol, mol)


# ---- save and load ------------------------------------------------------------------------------------
def test_a_saved_and_reloaded_batch_continues_bit_for_bit(water, tmp_path):
    from metropolismontecarlo_amd import checkpoint
    a, R = water, 3
    sol = sr.dipole(a)
    mol = placed_in_the_water(a, sol)
    path = str(tmp_path / "solute.ckpt")

    def first_leg(b):
        b.set_option("device_moves", 1)
        b.set_solute(sol, mol)
        e0 = b.potential_ewald(as_array=True)["energy"].copy()
        return b.run(70, T, DR, DPHI, seed=8, energies=e0, n_threads=2)[0]

    def second_leg(b, e):
        b.set_option("trace_steps", 60)
        e2, _ = b.run(60, T, DR, DPHI, seed=9, energies=e, n_threads=2)
        return e2.tobytes(), b.get_trace(60)[0].tobytes(), b.get_trace(60)[1].tobytes(), b.get_state().tobytes()
    with make_batch(a, R) as b:
        e1 = first_leg(b)
        b.save(path, extra=dict(energies=e1))
        straight = second_leg(b, e1)
    head = checkpoint.read_header(path)
    assert head["info"]["solute_on"] == 1 and head["info"]["solute_hash"] == scr.solute_hash(sol, mol)
    with make_batch(a, R) as b:                      # a fresh batch, no solute: load sets it
        b.set_option("device_moves", 1)
        extra = b.load(path)
        got = b.get_solute()
        assert got[1].tobytes() == mol.tobytes() and got[0].charge.tobytes() == sol.charge.tobytes()
        assert got[0].eps.tobytes() == sol.eps.tobytes() and got[0].sig.tobytes() == sol.sig.tobytes()
        assert second_leg(b, extra["energies"]) == straight
    with make_batch(a, R) as b:                      # ... and one that holds another solute
        b.set_option("device_moves", 1)
        b.set_solute(sr.cation(a), placed_in_the_water(a, sr.cation(a)))
        extra = b.load(path)
        assert second_leg(b, extra["energies"]) == straight
    # the library itself: records into a batch with no solute, or with another one, are refused
    with make_batch(a, R) as src:
        first_leg(src)
        info, rec = src.state_info(), src.get_state()
    other = structs.Solute("d", sol.offsets, sol.charge, sol.eps * 1.0000001, sol.sig)
    for setup in (lambda b: None, lambda b: (b.set_solute(other, mol), b.recip_long())):
        with make_batch(a, R) as b:
            b.set_option("device_moves", 1)
            setup(b)
            before = b.get_state().tobytes()
            with pytest.raises(_lib.MMCError, match="MMC_ERR_STATE.*solute"):
                b.set_state(info, rec)
            assert b.get_state().tobytes() == before


def test_save_keeps_its_own_names_and_load_reaches_a_stale_state(water, tmp_path):
    """The solute's arrays travel among the file's `extra` under names that are the file's own: a
    caller's array of such a name is refused, and load returns the caller's arrays only.  A state saved
    while S(k) awaited its rebuild loads into a batch that holds the same solute and a fresh S(k)."""
    a, R = water, 2
    sol = sr.dipole(a)
    mol = placed_in_the_water(a, sol)
    path = str(tmp_path / "stale.ckpt")
    with make_batch(a, R) as b:
        b.set_option("device_moves", 1)
        b.set_solute(sol, mol)
        assert b.state_info().s_stale
        with pytest.raises(ValueError, match="solute_mol"):
            b.save(path, extra=dict(solute_mol=np.zeros(3)))
        b.save(path, extra=dict(mine=np.arange(3)))
        e0 = b.potential_ewald(as_array=True)["energy"].copy()
        want = b.run(40, T, DR, DPHI, seed=3, energies=e0)[0].tobytes()
    for charged_before in (True, False):
        with make_batch(a, R) as b:
            b.set_option("device_moves", 1)
            if charged_before:
                b.set_solute(sol, mol)
            else:        # an uncharged solute of the same hash cannot be: another one, S(k) fresh
                b.set_solute(sr.methane(a), placed_in_the_water(a, sr.methane(a)))
            b.recip_long()
            extra = b.load(path)
            assert sorted(extra) == ["mine"] and extra["mine"].tolist() == [0, 1, 2]
            info = b.state_info()
            assert info.s_stale and info.solute_on and info.solute_hash == scr.solute_hash(sol, mol)
            e0 = b.potential_ewald(as_array=True)["energy"].copy()
            assert b.run(40, T, DR, DPHI, seed=3, energies=e0)[0].tobytes() == want
