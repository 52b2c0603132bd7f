"""CPU tests of bench.py's bookkeeping: the roofline object (what a launch's duration is when
launches overlap, which resource `binding` names), the algorithmic byte and flop counts of SURVEY
section 8(d), and the shapes the bench derives from a replica count."""
import argparse
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import common  # noqa: E402


def fake(streams, launches=40, elapsed=0.0102, span_us=350.0, timed=8):
    st = {"launches": launches, "moves": 32768 * launches, "timed_launches": timed,
          "kernel_ms": span_us * 1e-3 * timed}
    return {"st": st, "elapsed": elapsed, "streams": streams}


ARGS = argparse.Namespace(kernel=3, no_events=False)


def test_survey_counts():
    # 78.7 KB per trial move and 111.1 KB / 3.5e7 flop per full evaluation at 750 molecules
    assert bench.algorithmic_bytes_per_move(750, 30.0) == pytest.approx(78657, rel=1e-4)
    assert bench.algorithmic_bytes_full_eval(750) == 36 * 2250 + 24 * 750 + 36 * 337
    assert bench.algorithmic_flops_full_eval(750, 30.0) == pytest.approx(3.5e7, rel=0.02)


def test_launch_duration_is_cost_when_launches_overlap():
    two = bench.roofline_object(fake(2), 65536, ARGS, {"groups": 2}, 750, 30.0, 1)
    one = bench.roofline_object(fake(1, span_us=262.0), 65536, ARGS, {"groups": 2}, 750, 30.0, 1)
    # two streams: cost = timed region / launches, the event span is reported beside it
    assert two["avg_launch_us"] == pytest.approx(1e6 * 0.0102 / 40)
    assert two["launch_span_us"] == pytest.approx(350.0) and "wall time / launches" in two["avg_launch_us_is"]
    # one stream: the event duration IS the cost
    assert one["avg_launch_us"] == pytest.approx(262.0) and "HIP events" in one["avg_launch_us_is"]
    for r in (two, one):
        assert r["kernel"] == "k_move_eval_wave" and r["bound"] == "hbm" and r["peak"] == 8000.0
        assert r["frac"] == pytest.approx(r["achieved"] / 8000.0)
        assert r["achieved"] == pytest.approx(bench.algorithmic_bytes_per_move(750, 30.0) * 32768
                                              / (r["avg_launch_us"] * 1e-6) / 1e9)


def test_steps_per_launch_is_read_from_the_counts():
    st = {"launches": 10, "moves": 30720 * 8 * 10, "timed_launches": 0, "kernel_ms": 0.0}
    r = bench.roofline_object({"st": st, "elapsed": 0.017, "streams": 2}, 61440, ARGS, {"groups": 2}, 750, 30.0, 1)
    assert r["steps_per_launch"] == 8 and r["moves_per_launch"] == 30720 * 8


def test_binding_block_names_the_larger_fraction_and_stays_below_one():
    import glob
    import json
    shape = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_traffic.json")))
    mpl = int(json.load(open(shape[-1]))["moves_per_launch"]) if shape else 32768   # the committed launch shape
    R = 61440 if mpl % 30720 == 0 else 65536
    st = {"launches": 40, "moves": mpl * 40, "timed_launches": 8, "kernel_ms": 0.35 * 8 * mpl / 32768}
    r = bench.roofline_object({"st": st, "elapsed": 40 * 250e-6 * mpl / 32768, "streams": 2}, R, ARGS,
                              {"groups": 2}, 750, 30.0, 1)
    b = r.get("binding")
    if b is None:
        pytest.skip("no committed PMC summary for this launch shape under profiles/")
    v, h = b["fp64_valu_issue"], b["hbm"]
    assert v["peak"] == pytest.approx(1024 * v["clock_ghz"] / 4.0)
    assert v["achieved"] == pytest.approx(v["valu_insts_per_move"] * mpl / (r["avg_launch_us"] * 1e-6) / 1e9)
    assert 0 < v["frac"] <= 1.0 and 0 < h["frac"] <= 1.0
    cands = {"fp64_valu_issue": v["frac"]}
    if "access_pattern" in b:   # the kernel's loads and stores without arithmetic: their time / the launch's
        assert 0 < b["access_pattern"]["frac"] <= 1.0
        assert b["access_pattern"]["frac"] == pytest.approx(b["access_pattern"]["floor_us"] / r["avg_launch_us"])
        cands["hbm_access_pattern"] = b["access_pattern"]["frac"]
    assert b["bound"] == max(cands, key=cands.get) and b["frac"] == pytest.approx(max(cands.values()))
    assert "not measured in this run" in b["counters_source"]


def test_shapes():
    a = argparse.Namespace(groups=0, threads=8, steps=None, warmup=None, zero_copy_moves=-1)
    big, small = bench.shape_for(65536, a), bench.shape_for(32, a)
    assert big["groups"] == 2 and big["steps"] == 600 and big["warmup"] == 64 and big["prewarm"] == 56
    assert small["threads"] == 4 and small["steps"] == 3000 and bench.shape_for(1, a)["groups"] == 1
    assert bench.default_parts(65536, 750) == 1 and bench.default_parts(32, 750) == 5
    assert bench.server_lat_parts(1, 750) == 16 and bench.server_lat_parts(1, 10000) == 84
    assert bench.server_lat_parts(512, 750) == 0
    assert bench.kernel_name(3, 32768, 1) == "k_move_eval_wave" and bench.kernel_name(3, 32, 5) == "k_move_eval_fast"


def test_a_call_whose_last_launch_is_shorter_still_gets_its_binding_block():
    """The driver's `--steps 20`: launches of 8 + 8 + 4 steps.  The committed counters belong to the
    8-step launch; per move they hold for the call's average launch."""
    import glob
    import json
    shape = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_traffic.json")))
    if not shape or int(json.load(open(shape[-1]))["moves_per_launch"]) != 30720 * 8:
        pytest.skip("the committed counters are not those of 8-step launches of 30720 replicas")
    st = {"launches": 6, "moves": 61440 * 20, "timed_launches": 2, "kernel_ms": 4.4}
    r = bench.roofline_object({"st": st, "elapsed": 0.0090, "streams": 2}, 61440, ARGS, {"groups": 2}, 750, 30.0, 1)
    assert r["steps_per_launch"] == 8 and r["moves_per_launch"] == pytest.approx(61440 * 20 / 6)
    b = r["binding"]
    assert 0 < b["frac"] <= 1.0 and b["bound"] in ("fp64_valu_issue", "hbm_access_pattern")
    assert b["hbm"]["bytes_per_move"] == pytest.approx(json.load(open(shape[-1]))["bytes_per_move"])
    assert b["access_pattern"]["floor_us"] == pytest.approx(b["access_pattern"]["frac"] * r["avg_launch_us"])


def test_steps_and_dump_outputs_arguments():
    a = bench.parse_args(["--gpus", "1", "--steps", "24", "--warmup", "0", "--dump-outputs", "out"])
    assert a.steps == 24 and a.warmup == 0 and a.dump_outputs == "out"
    assert bench.shape_for(61440, a)["steps"] == 24 and bench.shape_for(32, a)["steps"] == 24
    assert bench.parse_args([]).dump_outputs is None
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_dump_sample_is_fixed_and_seeded():
    s = bench.dump_sample(61440)
    assert len(s) == bench.DUMP_SAMPLE and len(set(s.tolist())) == len(s)
    assert list(s) == sorted(s) and 0 <= s.min() and s.max() < 61440
    assert np.array_equal(s, bench.dump_sample(61440))
    assert np.array_equal(bench.dump_sample(5), np.arange(5))


class _FakeBatch:
    """get_replica of a batch whose replica r holds r everywhere"""
    R, n_mol = 40, 3

    def get_replica(self, r):
        return (np.full((self.n_mol, 3), float(r)), np.full((3 * self.n_mol, 3), float(r)),
                np.full(337, r + 0.5j))


def test_timed_outputs_are_written_as_float_arrays(tmp_path):
    st = {"moves": 800, "trans_attempt": 400, "trans_accept": 300, "rot_attempt": 400, "rot_accept": 250,
          "overlaps": 3, "wall_ms": 1.5, "kernel_ms": 0.5}
    energies = -np.arange(40, dtype=np.float64)
    out = bench.timed_outputs(_FakeBatch(), energies, st, g0=1000)
    names = bench.write_outputs(str(tmp_path / "d"), out, "_rank1")
    assert sorted(names) == sorted(f"{k}_rank1.npy" for k in out)
    got = {k: np.load(tmp_path / "d" / f"{k}_rank1.npy") for k in out}
    assert all(v.dtype == np.float64 for v in got.values())
    assert np.array_equal(got["energy"], energies)
    assert got["run_counts"].tolist() == [800, 400, 300, 400, 250, 3]
    idx = bench.dump_sample(40)
    assert np.array_equal(got["sample_replica"], 1000 + idx)
    assert got["sample_com"].shape == (16, 3, 3) and got["sample_coords"].shape == (16, 9, 3)
    assert np.array_equal(got["sample_coords"][:, 0, 0], idx)
    assert got["sample_sumqexp"].shape == (16, 337, 2)
    assert np.array_equal(got["sample_sumqexp"][:, 0], np.stack([idx, np.full(16, 0.5)], axis=1))
    # float32 stays float32; anything else becomes float64; 64 MB in all is the limit
    bench.write_outputs(str(tmp_path / "e"), {"a": np.ones(3, np.float32), "b": np.arange(3)})
    assert np.load(tmp_path / "e" / "a.npy").dtype == np.float32
    assert np.load(tmp_path / "e" / "b.npy").dtype == np.float64
    with pytest.raises(ValueError):
        bench.write_outputs(str(tmp_path / "f"), {"x": np.zeros(bench.DUMP_LIMIT_BYTES // 8 + 1)})
    assert not (tmp_path / "f").exists()


def test_wave_map_of_the_headline_shape():
    """The map the oracle tests choose their replicas from: 61440 chains in two groups on 256 compute
    units are six units per wave; small batches under option "wave_wgs" run several, unevenly."""
    w = common.wave_units(30720)
    assert len(w) == 5120 and {len(x) for x in w} == {6} and w[1][:2] == [1, 5121]
    assert sorted(u for x in w for u in x) == list(range(30720))
    assert [len(x) for x in common.wave_units(12, 2)] == [2] * 4 + [1] * 4
    assert [len(x) for x in common.wave_units(13, 1)] == [4, 3, 3, 3]
    assert [len(x) for x in common.wave_units(12)] == [1] * 12              # a wave per unit
    pos = common.replicas_by_wave_position(25, 2, wave_wgs=1)
    assert list(pos) == [0, 4, 8, 11, 12, 16, 20, 21, 24]
    assert pos[24] == "group 1, wave 0, unit 4 of 4" and pos[21] == "group 1, wave 1, unit 3 of 3"
    assert list(common.replicas_by_wave_position(24, 2)) == [0, 11, 12, 23]
