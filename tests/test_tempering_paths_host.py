"""Host side of tests/test_gpu_tempering_paths.py and of the ladder rows of test_gpu_tempering.py
(no GPU): the conditions under which their ladders matter, from the chains stepped by the CPU
oracle -- so that a seed or a ladder cannot stop probing silently.  Seeds and ladders are settled
here."""
import numpy as np
import pytest

import test_gpu_multi_record as mr
import test_gpu_tempering as tp
import test_gpu_tempering_paths as pp


@pytest.mark.parametrize("wolf", [False, True])
def test_every_laddered_chain_has_a_replica_per_group_the_ladder_changes(wolf):
    """The chain every row of tp.PATHS runs: in each group of four a replica decides otherwise at
    the scalar of the call than at temps[r], and a replica of the second group otherwise at the
    temperature of its place in the first -- what an index local to the group would read."""
    def flags(r, T):
        return [f for _, f in tp.ladder_replay(r, T, wolf)["trace"]]

    half = tp.L_R // 2
    changed = [r for r in range(tp.L_R) if flags(r, tp.L_TEMPS[r]) != flags(r, tp.L_SCALAR)]
    assert {r // half for r in changed} == {0, 1}, changed
    assert [r for r in range(half, tp.L_R) if flags(r, tp.L_TEMPS[r]) != flags(r, tp.L_TEMPS[r - half])]


@pytest.mark.parametrize("case", pp.D_CASES)
def test_the_ladder_changes_chains_of_both_groups(case):
    """Per variant and style: in each group a replica's accept trace at temps[r] is not its trace at
    mr.T; in the second group one's is not its trace at temps[r - 12] either; and the two-group
    split of the 24 distinct temperatures is what those conditions assume."""
    assert len(set(pp.D_TEMPS.tolist())) == mr.R and pp.D_GROUPS * (mr.R // pp.D_GROUPS) == mr.R
    changed = pp.chains_the_ladder_changes(case)
    assert {pp.group_of(r) for r in changed} == set(range(pp.D_GROUPS)), (case, changed)
    assert pp.chains_a_group_local_index_changes(case), case
    for r in changed:
        assert 0 < sum(pp.accepts(pp.nist4_replay(case, r, pp.D_TEMPS[r]))) < mr.N_STEPS, (case, r)


@pytest.mark.parametrize("case", pp.D_CASES)
def test_the_lone_last_launch_decides_by_its_own_temperature(case):
    """8 + 8 + 1: some replica's step 16, reached under temps[r], is accepted at temps[r] and
    rejected at mr.T or the reverse -- a one-step launch reading the scalar could not pass."""
    assert pp.D_SHORT % 8 == 1 and pp.D_SHORT < mr.N_STEPS
    assert pp.last_launch_deciders(case), case


def test_the_controller_tells_the_coldest_rung_from_the_hottest():
    """run_chains(adjust=True): after two sweeps stepped by the oracle at temps[r], the host mirror
    of Adjust! leaves the coldest and the hottest rung different dr_max, neither the one it began
    with."""
    cold, hot = pp.oracle_step_sizes(0), pp.oracle_step_sizes(tp.L_R - 1)
    assert cold[0] != hot[0] and cold[0] != pp.Q_DR and hot[0] != pp.Q_DR, (cold, hot)


@pytest.mark.parametrize("wolf", [False, True])
def test_the_ladder_spacing_accepts_and_rejects_swaps_in_both_styles(wolf):
    """run_exchange's paths: stepped by the oracle, the 6 rounds accept and reject swaps -- the
    Ewald chains (kernel 1, the server and the one-step kernel run the same ones) and the Wolf
    chains, whose energies are their own, on the same spacing."""
    o = tp.oracle_ladder_run(wolf)
    assert sum(o["accept"]) >= 1 and sum(o["attempt"]) - sum(o["accept"]) >= 1, o
    assert np.array(o["temps"]).shape == (tp.X_ROUNDS + 1, tp.X_R)
