"""A whole call in one launch per group (option "whole_call") against launches of eight steps.

The bench's flagship batch -- 61440 chains of NIST configuration 4 in two groups, the move kernel
deciding, launches of eight steps whose waves take their units from a queue -- and the same batch
with option whole_call = 1, where a call of up to 32 steps takes ONE launch per group.  Both forms
must run the same chains: calls of 20, 7, 1 and 33 steps back to back, so that each call continues
the random streams, the S-buffer parity and the ring of device-made proposals of the one before."""
import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu

RCUT = 10.0
R = 61440
CALLS = (20, 7, 1, 33)
COUNTS = ("moves", "trans_attempt", "trans_accept", "rot_attempt", "rot_accept", "overlaps")


def _launches(n, whole, G=2):
    per = 32 if whole else 8
    return G * -(-n // per)


def _run_calls(a, whole, inject=0):
    from metropolismontecarlo_amd import structs
    from metropolismontecarlo_amd.device import Batch
    check = sorted(set(common.replicas_by_wave_position(R, 2, 0, common.device_cu_count()))
                   | set(np.random.default_rng(5).choice(R, 24, replace=False).tolist()))
    with Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
               5.6 / a["box"], structs.factor, RCUT, RCUT) as b:
        b.set_option("kernel", 3)
        b.set_option("device_moves", 1)
        b.set_option("accept_on_device", -1)
        if whole is not None:
            b.set_option("whole_call", whole)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        stats = []
        for k, n in enumerate(CALLS):
            if inject and k == 0:
                b.set_option("inject_torn", inject)
            e, st = b.run(n, 298.15, 0.316555789, 0.05, seed=4242, energies=e, n_groups=2,
                          n_parts=0, time_kernels=4, n_threads=2, n_streams=2)
            assert st["device_decisions"] == R * n and st["server_steps"] == 0, st
            stats.append(st)
        t = b.potential_ewald(as_array=True)["energy"]
        reps = {r: b.get_replica(r) for r in check}
    return e, t, stats, reps


@pytest.fixture(scope="module")
def runs():
    a = common.nist_arrays(4, "unwrapped")
    return {"eight": _run_calls(a, None), "whole": _run_calls(a, 1), "whole_torn": _run_calls(a, 1, inject=7)}


def test_launch_counts(runs):
    for form, whole in (("eight", lambda n: False), ("whole", lambda n: True), ("whole_torn", lambda n: True)):
        for n, st in zip(CALLS, runs[form][2]):
            assert st["launches"] == _launches(n, whole(n)), (form, n, st["launches"])
            assert st["moves"] == R * n


def test_same_chains_in_both_forms(runs):
    e8, t8, s8, r8 = runs["eight"]
    for form in ("whole", "whole_torn"):
        e, t, s, reps = runs[form]
        for a_, b_ in zip(s8, s):
            assert [a_[k] for k in COUNTS] == [b_[k] for k in COUNTS], form
        # the same device state: coordinates and S(k) bit for bit
        for r, (com, coords, sk) in reps.items():
            assert np.array_equal(com, r8[r][0]) and np.array_equal(coords, r8[r][1]), (form, r)
            assert np.array_equal(sk, r8[r][2]), (form, r)
        assert np.array_equal(t, t8), form
        # running totals: the steps of a launch are summed in another grouping
        assert np.max(np.abs(e - e8) / np.abs(e8)) < 1e-12, form


def test_running_energies_against_a_recompute(runs):
    for form in ("eight", "whole", "whole_torn"):
        e, t, _, _ = runs[form]
        assert np.max(np.abs(e - t) / np.abs(t)) < 1e-12, form


def test_torn_records(runs):
    for form in ("eight", "whole"):
        assert all(st["torn_records"] == 0 for st in runs[form][2]), form
    # seven corrupted copies in the first call: each refused and read again, the chains unchanged
    st = runs["whole_torn"][2]
    assert st[0]["torn_records"] == 7 and all(x["torn_records"] == 0 for x in st[1:])
