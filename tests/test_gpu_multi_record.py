"""What a launch of several steps sends -- dU of the accepted steps, the accept / overlap masks, the
move kinds and no virial -- against the one-step kernel.

The MULTI instantiations of k_move_eval_wave compute no LJ virial, reduce four sums instead of six
and make the record's checksum only in the step that stores it.  Every sum the decision reads must
keep its bits, so a chain run at eight steps per launch (the kernel decides) and the same chain run
with accept_on_device = 0 -- one step per launch through the MULTI = false instantiation, the host
decides -- must be the same chain: the six counts of the call, and centres of mass, coordinates and
S(k) of every replica bit for bit.  The running energies may differ in the grouping of the sum over
a launch's accepted steps (1e-12 relative, the rule of test_gpu_whole_call.py) and must agree with a
recompute of the final state to 1e-9 relative: the batch's own potential_ewald (potential_wolf for
the Wolf chains, whose running energy is the Wolf total), and for the Ewald cases the oracle's.

NIST configuration 4 (750 molecules, r_cut 10 A): about 117 gated neighbours, so two rounds of the
pair loop with idle lanes in the second.  R = 24 in two groups with wave_wgs = 1: four waves take
twelve units per launch, three each, the second and third by ticket.  20 steps: launches of 8 + 8 + 4.
"unwrapped" centres of mass take the molecule-image form of the pair loop (IMG = true), "reference"
ones -- molecules stored broken across the box -- the per-atom minimum image."""
import functools

import numpy as np
import pytest

import common
from common import rel

pytestmark = pytest.mark.gpu

RCUT, T, DPHI = 10.0, 298.15, 0.3
R, N_STEPS, SEED, REPLICA0 = 24, 20, 20240, 5
DR, DR_OVERLAP = 0.316555789, 3.0
COUNTS = ("moves", "trans_attempt", "trans_accept", "rot_attempt", "rot_accept", "overlaps")
ON_DEVICE = dict(kernel=2, persistent=0, accept_on_device=1, steps_per_launch=8, whole_call=0, wave_wgs=1)
ON_HOST = dict(kernel=2, persistent=0, accept_on_device=0, wave_wgs=1)

CASES = {"ewald-unwrapped": ("unwrapped", "ewald", DR), "ewald-reference": ("reference", "ewald", DR),
         "wolf-unwrapped": ("unwrapped", "wolf", DR), "wolf-reference": ("reference", "wolf", DR),
         "ewald-unwrapped-overlaps": ("unwrapped", "ewald", DR_OVERLAP)}


def _run(a, style, dr, opts):
    """One call of N_STEPS on a fresh batch.  Returns the running energies, the recomputed totals of
    the final state, the call's stats and every replica's (com, coords, S)."""
    from metropolismontecarlo_amd import structs
    from metropolismontecarlo_amd.device import Batch
    with Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
               5.6 / a["box"], structs.factor, RCUT, RCUT) as b:
        b.set_option("device_moves", 1)
        for k, v in opts.items():
            b.set_option(k, v)
        total = b.potential_ewald
        if style == "wolf":
            b.recip_long()
            b.set_coulomb_style("wolf")
            total = b.potential_wolf
        e0 = total(as_array=True)["energy"].copy()
        e1, st = b.run(N_STEPS, T, dr, DPHI, seed=SEED, energies=e0, n_groups=2, n_parts=1, n_threads=2,
                       replica0=REPLICA0)
        final = [b.get_replica(r) for r in range(R)]
        t1 = total(as_array=True).copy()
    return e1, t1, st, final


@functools.lru_cache(maxsize=None)
def runs(case):
    variant, style, dr = CASES[case]
    a = common.nist_arrays(4, variant)
    return _run(a, style, dr, ON_DEVICE), _run(a, style, dr, ON_HOST)


@functools.lru_cache(maxsize=None)
def oracle_overlaps(case):
    """Overlaps each chain meets in the call, stepped by the oracle on the host."""
    from oracle import oracle as orc
    from test_gpu_replay_paths import replay
    variant, style, dr = CASES[case]
    a = common.nist_arrays(4, variant)
    return [replay(orc, a, REPLICA0 + r, [(N_STEPS, SEED, 0)], T, dr, DPHI, RCUT, wolf=style == "wolf")["n_ovl"]
            for r in range(R)]


def _same_bits(x, y):
    return x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("case", list(CASES))
def test_eight_steps_per_launch_run_the_one_step_chains(case):
    (e_d, t_d, st_d, fin_d), (e_h, t_h, st_h, fin_h) = runs(case)
    assert st_d["launches"] == 2 * 3 and st_d["device_decisions"] == R * N_STEPS, st_d
    assert st_h["launches"] == 2 * N_STEPS and st_h["device_decisions"] == 0, st_h
    assert [st_d[k] for k in COUNTS] == [st_h[k] for k in COUNTS], (st_d, st_h)
    n_acc = st_d["trans_accept"] + st_d["rot_accept"]
    assert 0 < n_acc < R * N_STEPS and st_d["rot_attempt"] > 0    # all three words of the record carry something
    for r in range(R):
        for x, y, what in zip(fin_d[r], fin_h[r], ("com", "coords", "S(k)")):
            assert _same_bits(x, y), (case, r, what)
    assert t_d.tobytes() == t_h.tobytes(), case
    # the pre-summed dU of a launch: the same terms in another grouping
    print(case, "running energies, device against host:", np.max(np.abs(e_d - e_h) / np.abs(e_h)))
    assert np.max(np.abs(e_d - e_h) / np.abs(e_h)) < 1e-12, case
    print(case, "running energies against the recompute:", np.max(np.abs(e_d - t_d["energy"]) / np.abs(t_d["energy"])))
    assert np.max(np.abs(e_d - t_d["energy"]) / np.abs(t_d["energy"])) < 1e-9, case


@pytest.mark.parametrize("case", ["ewald-unwrapped", "ewald-reference", "ewald-unwrapped-overlaps"])
def test_running_energies_against_the_oracle_recompute(case):
    """potential_ewald of the oracle on the downloaded final state of the replicas that took a wave's
    first, second and third unit."""
    from oracle import oracle as orc
    variant, _, _ = CASES[case]
    a = common.nist_arrays(4, variant)
    (e_d, _, _, fin_d), _ = runs(case)
    for r in (0, 3, 4, 11, 12, 23):
        com, coords, _ = fin_d[r]
        s = common.oracle_system(dict(a, com=com, coords=coords))
        to = orc.potential_ewald(s, orc.Ewald(5.6 / s.box, 5, 27, s.box), RCUT, RCUT)
        assert rel(e_d[r], to["energy"]) < 1e-9, (case, r, e_d[r], to["energy"])


def test_overlaps_travel_through_the_record():
    """dr_max = 3 A: the oracle's chains meet overlaps in these 20 steps (the precondition), and the
    launch's record reports exactly those."""
    n_ovl = oracle_overlaps("ewald-unwrapped-overlaps")
    assert sum(n_ovl) >= 1, n_ovl
    (_, _, st_d, _), (_, _, st_h, _) = runs("ewald-unwrapped-overlaps")
    assert st_d["overlaps"] == sum(n_ovl) and st_h["overlaps"] == sum(n_ovl), (st_d["overlaps"], n_ovl)


# ---- kernel timing and launch counts -----------------------------------------------------------------
# time_kernels = 1 brackets every launch of a group with the group's pair of events, on both driver
# paths.  (n_groups, n_steps): launches of 8 + 8 + 4 per group, one group alone (its next launch is
# enqueued at once, nothing is held back), exactly one launch per group (the last is the first) and a
# single step.  Timing must change nothing but the timing fields.
TIMING_SHAPES = [(2, 20), (1, 20), (2, 8), (2, 1)]
TIMING_MODES = {"device": ON_DEVICE, "host": ON_HOST}


def _run_timed(opts, n_groups, n_steps, time_kernels):
    """One call on a fresh batch of the "ewald-unwrapped" case: energies, stats, final states."""
    from metropolismontecarlo_amd import structs
    from metropolismontecarlo_amd.device import Batch
    a = common.nist_arrays(4, "unwrapped")
    with Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
               5.6 / a["box"], structs.factor, RCUT, RCUT) as b:
        b.set_option("device_moves", 1)
        for k, v in opts.items():
            b.set_option(k, v)
        e0 = b.potential_ewald(as_array=True)["energy"].copy()
        e1, st = b.run(n_steps, T, DR, DPHI, seed=SEED, energies=e0, n_groups=n_groups, n_parts=1, n_threads=2,
                       replica0=REPLICA0, time_kernels=time_kernels)
        final = [b.get_replica(r) for r in range(R)]
    return e1, st, final


@pytest.mark.parametrize("n_groups,n_steps", TIMING_SHAPES)
@pytest.mark.parametrize("mode", list(TIMING_MODES))
def test_every_launch_is_timed_and_timing_changes_nothing(mode, n_groups, n_steps):
    opts = TIMING_MODES[mode]
    e_t, st_t, fin_t = _run_timed(opts, n_groups, n_steps, 1)
    e_0, st_0, fin_0 = _run_timed(opts, n_groups, n_steps, 0)
    # the kernel decides: launches of up to eight steps; the host decides: a launch per step
    want = n_groups * ((n_steps + 7) // 8 if mode == "device" else n_steps)
    print(mode, n_groups, n_steps, "launches", st_t["launches"], "timed", st_t["timed_launches"], "kernel_ms",
          st_t["kernel_ms"])
    assert st_t["launches"] == want and st_0["launches"] == want, (st_t, st_0)
    assert st_t["device_decisions"] == (R * n_steps if mode == "device" else 0), st_t
    assert st_t["timed_launches"] == st_t["launches"], st_t
    assert st_t["kernel_ms"] > 0, st_t
    assert st_0["timed_launches"] == 0 and st_0["kernel_ms"] == 0, st_0
    assert [st_t[k] for k in COUNTS] == [st_0[k] for k in COUNTS], (st_t, st_0)
    assert st_t["moves"] == R * n_steps, st_t
    for r in range(R):
        for x, y, what in zip(fin_t[r], fin_0[r], ("com", "coords", "S(k)")):
            assert _same_bits(x, y), (mode, n_groups, n_steps, r, what)
    assert _same_bits(e_t, e_0), (mode, n_groups, n_steps)   # timing changes no sum
