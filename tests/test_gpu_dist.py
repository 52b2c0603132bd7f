"""The product's N>1 launch path, rehearsed on one GPU: the driver's own command line
`python -m torch.distributed.run --nproc-per-node 2 bench.py --gpus 2 ...` with
MMC_DIST_BACKEND=gloo, so that both ranks share cuda:0 and the final reduction runs over gloo (on
the 8-GPU node the same code runs one rank per GPU over RCCL).  Launched by tests/conftest.py
before this process touches the GPU; checked here:

  * the JSON contract line of rank 0 (n_gpus, moves, weak scaling, roofline object),
  * running totals equal a recompute on every rank (energy_drift_rel),
  * the 2 x 64 chains are THE SAME chains as one process running global indices 0..127:
    trajectories depend on (seed, global replica index) only -- identical accept counts and the
    same energy sum.

No scaling claim is made from this: two ranks share one device."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu


def load(out, name):
    rc = open(os.path.join(out, name + ".rc")).read().strip()
    err = open(os.path.join(out, name + ".err")).read()
    assert rc == "0", (name, rc, err[-2000:])
    lines = [l for l in open(os.path.join(out, name + ".json")).read().splitlines() if l.startswith("{")]
    assert len(lines) == 1, (name, lines, err[-2000:])      # ONE JSON line, from rank 0 only
    return json.loads(lines[0])


def test_two_ranks_share_nothing_but_the_final_reduction(dist_rehearsal):
    two, one = load(dist_rehearsal, "two"), load(dist_rehearsal, "one")
    assert two["n_gpus"] == 2 and one["n_gpus"] == 1
    assert two["scaling"] == "weak" and two["unit"] == "moves/s" and two["dtype"] == "f64"
    assert two["steps"] == 20 and two["warmup"] == 5
    assert two["config"]["replicas_per_gpu"] == 64 and two["config"]["replicas_total"] == 128
    assert one["config"]["replicas_total"] == 128
    moves = 2 * 64 * 20
    assert abs(two["value"] * two["ms_per_step"] * 1e-3 * 20 - moves) < 1e-6 * moves   # value = moves / time
    for d in (two, one):
        assert d["energy_drift_rel"] < 1e-12
        assert d["roofline"]["kernel"] in ("k_move_eval_wave", "k_move_eval_fast", "k_move_eval_lat")
        assert d["roofline"]["frac"] > 0
        assert d["vs_baseline"] is None and d["higher_is_better"] is True
    # the same 128 chains either way
    assert two["acceptance"] == one["acceptance"]
    assert two["overlaps"] == one["overlaps"]
    e2, e1 = two["energy_mean_per_replica"], one["energy_mean_per_replica"]
    assert abs(e2 - e1) < 1e-13 * abs(e1), (e2, e1)


def test_two_ranks_of_32_chains_run_the_move_server(dist_rehearsal):
    """BASELINE configs[2] is 256 chains over 8 GPUs = 32 per rank: that shape runs on the
    persistent move server (host threads answering control words), here with two ranks at once."""
    d = load(dist_rehearsal, "two32")
    assert d["n_gpus"] == 2 and d["config"]["replicas_per_gpu"] == 32 and d["config"]["replicas_total"] == 64
    assert "move server" in d["config"]["driver"]
    assert d["energy_drift_rel"] < 1e-12 and d["torn_result_records"] == 0
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 * 200 - 64 * 200) < 1e-6 * 64 * 200
    assert 0.5 < d["acceptance"] < 0.95


def test_two_ranks_in_the_headline_s_mode_run_the_same_chains_as_one(dist_rehearsal):
    """The mode the headline runs in -- the move kernel takes the accept decision, a launch takes a
    group through eight steps -- under two ranks of 10240 chains, against one process running global
    indices 0..20479: the same chains (accept count, energy sum), whatever the split."""
    two, one = load(dist_rehearsal, "two_dev"), load(dist_rehearsal, "one_dev")
    for d in (two, one):
        assert d["config"]["accept_decision"] == "move kernel" and d["roofline"]["steps_per_launch"] == 8
        assert d["roofline"]["kernel"] == "k_move_eval_wave"
        assert d["energy_drift_rel"] < 1e-12 and d["torn_result_records"] == 0
        assert d["config"]["replicas_total"] == 20480 and d["steps"] == 24
    assert two["n_gpus"] == 2 and one["n_gpus"] == 1
    assert two["acceptance"] == one["acceptance"] and two["overlaps"] == one["overlaps"]
    e2, e1 = two["energy_mean_per_replica"], one["energy_mean_per_replica"]
    assert abs(e2 - e1) < 1e-13 * abs(e1), (e2, e1)


def _dumped(directory, suffix=""):
    import numpy as np
    names = ("energy", "run_counts", "sample_replica", "sample_com", "sample_coords", "sample_sumqexp")
    return {k: np.load(os.path.join(directory, f"{k}{suffix}.npy")) for k in names}


def test_dumped_outputs_are_the_timed_call_s_and_repeat_from_run_to_run(dist_rehearsal):
    """`bench.py --dump-outputs DIR`: the timed call's outputs, written after its timing.  The energies
    are the ones the JSON line averages, the counts are the JSON line's, the same command writes the
    same outputs again, and two ranks write the same chains as one process."""
    import numpy as np
    one, again, two = (load(dist_rehearsal, n) for n in ("one_dev", "one_dev_again", "two_dev"))
    d1 = _dumped(os.path.join(dist_rehearsal, "one_dev_out"))
    d1b = _dumped(os.path.join(dist_rehearsal, "one_dev_again_out"))
    assert sorted(one["dumped_outputs"]["files"]) == sorted(f"{k}.npy" for k in d1)
    for k, v in d1.items():
        assert v.dtype == np.float64, k
        assert np.array_equal(v, d1b[k]), k               # same arguments: the same outputs
    R, n_mol = 20480, 750
    assert d1["energy"].shape == (R,) and np.isfinite(d1["energy"]).all()
    assert abs(d1["energy"].mean() - one["energy_mean_per_replica"]) < 1e-13 * abs(one["energy_mean_per_replica"])
    moves, t_att, t_acc, r_att, r_acc, overlaps = d1["run_counts"]
    assert moves == R * 24 == t_att + r_att and overlaps == one["overlaps"]
    assert (t_acc + r_acc) / moves == one["acceptance"]
    assert d1["sample_com"].shape == (16, n_mol, 3) and d1["sample_coords"].shape == (16, 3 * n_mol, 3)
    assert d1["sample_sumqexp"].shape == (16, 337, 2)
    idx = d1["sample_replica"].astype(np.int64)
    assert len(set(idx.tolist())) == 16 and idx.min() >= 0 and idx.max() < R
    # two ranks of 10240: each writes its own shard of the same 20480 chains
    d2 = [_dumped(os.path.join(dist_rehearsal, "two_dev_out"), f"_rank{k}") for k in (0, 1)]
    e2 = np.concatenate([d["energy"] for d in d2])
    assert np.abs(e2 - d1["energy"]).max() <= 1e-12 * np.abs(d1["energy"]).max()
    assert np.array_equal(d2[0]["run_counts"] + d2[1]["run_counts"], d1["run_counts"])
    assert d2[1]["sample_replica"].min() >= 10240 and d2[0]["sample_replica"].max() < 10240


def test_dumped_bench_outputs_against_the_oracle(dist_rehearsal):
    """The state the headline's code path leaves behind, against the oracle: the sampled replicas
    of `bench.py --replicas 20480 ... --dump-outputs` (two units per wave) replayed through the three
    calls the bench made on its batch -- prewarm, warm-up, timed, each with its own seed, the
    Philox counter continuing from call to call.  Step counts and seeds are the bench's own."""
    import types
    import numpy as np
    import bench
    import common
    from metropolismontecarlo_amd import sharding
    from oracle import oracle as orc
    from test_gpu_batch import TOL, make_batch, oracle_replay
    one = load(dist_rehearsal, "one_dev")
    d = _dumped(os.path.join(dist_rehearsal, "one_dev_out"))
    R = one["config"]["replicas_total"]
    shape = bench.shape_for(R, types.SimpleNamespace(groups=0, threads=2, steps=one["steps"],
                                                     warmup=one["warmup"], zero_copy_moves=-1))
    assert one["config"]["prewarm_steps"] == shape["prewarm"] > 0
    calls = [(shape["prewarm"], sharding.run_seed(phase=2)), (shape["warmup"], sharding.run_seed(phase=0)),
             (shape["steps"], sharding.run_seed(phase=1))]
    a = common.nist_arrays(4, "unwrapped")        # the bench's system
    with make_batch(a, 1) as b:                   # the initial total every chain starts from
        e0 = b.potential_ewald(as_array=True)["energy"][0]
    for k, r in enumerate(d["sample_replica"].astype(np.int64)):
        o = oracle_replay(orc, a, int(r), calls, bench.TEMPERATURE, bench.DR_MAX, bench.DPHI_MAX)
        S = d["sample_sumqexp"][k, :, 0] + 1j * d["sample_sumqexp"][k, :, 1]
        assert np.abs(d["sample_com"][k] - o["com"]).max() < 2e-13, r
        assert np.abs(d["sample_coords"][k] - o["coords"]).max() < 2e-13, r
        assert np.abs(S - o["S"]).max() < 1e-11 * np.abs(o["S"]).max(), r
        assert abs((d["energy"][r] - e0) - o["e_acc"]) < TOL * 1e5, r
        assert 0 < o["n_acc"] < sum(n for n, _ in calls), r


def test_rccl_collective_behind_the_c_abi():
    """mmc_dist_*: the final reduction for hosts without torch.  A one-GPU box can form a
    communicator of ONE rank only (RCCL wants a GPU per rank): that still goes through
    ncclGetUniqueId / ncclCommInitRank / ncclAllReduce (sum and max, fp64) / ncclCommDestroy."""
    import ctypes as C
    import numpy as np
    from metropolismontecarlo_amd import _lib
    L = _lib.lib()
    ident = C.create_string_buffer(128)
    _lib.check(L.mmc_dist_unique_id(ident))
    assert any(ident.raw)
    d = C.c_void_p()
    _lib.check(L.mmc_dist_init(0, 1, ident, 0, C.byref(d)))
    sums = np.array([1.5, -2.25, 3e10, 0.0])
    mx = np.array([0.125, -7.0])
    dp = C.POINTER(C.c_double)
    for _ in range(3):
        _lib.check(L.mmc_dist_reduce(d, sums.ctypes.data_as(dp), 4, mx.ctypes.data_as(dp), 2))
    assert np.array_equal(sums, [1.5, -2.25, 3e10, 0.0]) and np.array_equal(mx, [0.125, -7.0])
    _lib.check(L.mmc_dist_reduce(d, None, 0, mx.ctypes.data_as(dp), 2))
    _lib.check(L.mmc_dist_destroy(d))
    # the same through sharding.reduce_observables
    from metropolismontecarlo_amd import sharding
    local = dict(moves=10, accepted=4, overlaps=0, energy_sum=-1.5, kernel_ms=2.0, launches=3)
    with sharding.RcclReducer(0, 1) as red:
        out, t = sharding.reduce_observables(local, 0.25, red)
    assert out["moves"] == 10 and out["energy_sum"] == -1.5 and t == 0.25
