"""Deletion energies (mmc_batch_deletion) on the rest of what k_deletion_wave reads or branches on,
against the oracle (test_gpu_deletion.py has the definition, the sums and the refusals):
  * the neighbour list emptied mid-scan, so that the pair sums add across process() calls;
  * separate LJ and Coulomb cutoffs (the prefilter takes the larger gate, the pair body its
    same_gate == false branch);
  * the committed state (coordinates, records, S buffer, box, kappa) after every path that changes
    it -- the cases of tests/test_gpu_widom_paths.py.
The oracle terms (deletion_ref.oracle_terms) recompute RecipLong from each replica's coordinates
(get_replica), so a stale or wrong S(k) buffer shows in d_recip, and a stale record in every term.
Tolerance: 1e-9 K plus 1e-13 of each term (common.widom_close), the overlap flag exact."""
import math

import numpy as np
import pytest

import common
import deletion_ref as ref

pytestmark = pytest.mark.gpu

T = 298.15
RC = 10.0
SEL8 = np.array([0, 63, 64, 301, 302, 511, 700, 749])


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def cfg4():
    return common.nist_arrays(4, "unwrapped")


def make_batch(a, R, lj=RC, qq=RC, recip=True):
    from metropolismontecarlo_amd import structs
    from metropolismontecarlo_amd.device import Batch
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
              5.6 / a["box"], structs.factor, lj, qq)
    if recip:
        b.recip_long()
    return b


def check_selected(orc, a, b, sel, what, lj=RC, qq=RC):
    """The selected molecules of every replica against the oracle on get_replica's configuration,
    and the sums against the fixed-order host sums of the returned rows."""
    res = b.deletion(T, sel=sel, details=True)
    for r in range(b.R):
        ref.check(orc, a, b, r, sel, res["du"][r], res["ovl"][r], lj, qq, what=what)
    esum, boltz, nfl = ref.host_sums(res["du"], res["ovl"], T)
    assert res["esum"].tobytes() == esum.tobytes(), what
    assert np.all(np.abs(res["boltz_sum"] - boltz) <= 1e-14 * np.abs(boltz)), what
    assert np.array_equal(res["n_flagged"], nfl), what
    return res


# ---- 8. the pair-list flush ---------------------------------------------------------------------
def test_neighbour_list_flush(orc):
    """2000 SPC/E molecules compressed to 0.06 / A^3 (32.2 A) with a 12.4 A cutoff: 430-520 COMs
    inside the gate of any molecule, so the scan of k_deletion_wave empties its list after a trip
    and goes on (asserted on the host, common.scan_flushes, the molecule itself left out): the pair
    sums add across process() calls."""
    from test_gpu_batch import _dense_water
    a = _dense_water(2000, rho=0.06)
    L, rc = float(a["box"]), 12.4
    assert rc < L / 2 and 5.6 / L * math.sqrt(rc * rc + 100) < 2.8
    com = np.asarray(a["com"])
    rng = np.random.default_rng(2000)
    sel = [int(i) for i in rng.permutation(2000) if common.scan_flushes(com, [com[i]], rc, L, exclude=int(i))][:24]
    assert len(sel) == 24
    sel = np.array(sel)
    for i in sel:
        assert common.scan_flushes(com, [com[i]], rc, L, exclude=int(i)), i
    with make_batch(a, 1, rc, rc) as b:
        check_selected(orc, a, b, sel, "flush", rc, rc)


# ---- 9. separate cutoffs ------------------------------------------------------------------------
@pytest.mark.parametrize("lj,qq", [(8.0, 10.0), (10.0, 8.0)])
def test_separate_cutoffs(lj, qq, cfg4, orc):
    sel = np.array([0, 1, 63, 64, 65, 127, 128, 200, 255, 256, 301, 400, 512, 640, 700, 749])
    with make_batch(cfg4, 1, lj, qq) as b:
        b.set_option("device_moves", 1)
        b.run(60, T, 0.3, 0.2, seed=99)
        check_selected(orc, cfg4, b, sel, (lj, qq), lj, qq)


# ---- 11. after every path that changes the committed state --------------------------------------
def test_after_host_decided_runs(cfg4, orc):
    """One step per launch, the host decides (persistent = 0, accept_on_device = 0)."""
    with make_batch(cfg4, 8) as b:
        for k, v in (("device_moves", 1), ("kernel", 2), ("persistent", 0), ("accept_on_device", 0)):
            b.set_option(k, v)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        e, st = b.run(37, T, 0.3, 0.2, seed=5, energies=e)
        assert st["device_decisions"] == 0 and st["trans_accept"] + st["rot_accept"] > 0
        check_selected(orc, cfg4, b, SEL8, "host-decided")


def test_after_kernel_decided_runs(cfg4, orc):
    """Eight steps per launch, the kernel decides, 24 replicas in two groups on one workgroup: the
    terms of every replica, and the chains go on bit for bit like a twin's that made no such call."""
    R, per_launch = 24, 8
    opts = (("device_moves", 1), ("kernel", 2), ("persistent", 0), ("accept_on_device", 1),
            ("steps_per_launch", per_launch), ("wave_wgs", 1))
    with make_batch(cfg4, R) as b, make_batch(cfg4, R) as tw:
        es = []
        for x in (b, tw):
            for k, v in opts:
                x.set_option(k, v)
            e = x.potential_ewald(as_array=True)["energy"].copy()
            e, st = x.run(3 * per_launch + 5, T, 0.3, 0.2, seed=6, energies=e, n_groups=2, n_parts=1)
            assert st["device_decisions"] == R * (3 * per_launch + 5)
            es.append(e)
        # the molecules each chain moved last are among those looked at
        check_selected(orc, cfg4, b, SEL8, per_launch)
        for x, k in ((b, 0), (tw, 1)):
            es[k], _ = x.run(2 * per_launch + 3, T, 0.3, 0.2, seed=7, energies=es[k], n_groups=2, n_parts=1)
        assert es[0].tobytes() == es[1].tobytes()
        for r in range(R):
            for u, v in zip(b.get_replica(r), tw.get_replica(r)):
                assert np.asarray(u).tobytes() == np.asarray(v).tobytes(), r


def test_after_the_latency_server(cfg4, orc):
    """One replica with the default options: the latency server runs the chain."""
    with make_batch(cfg4, 1) as b:
        b.set_option("device_moves", 1)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        e, st = b.run(150, T, 0.3, 0.2, seed=8, energies=e, n_groups=1)
        assert st["server_steps"] == 150
        moved = np.nonzero(np.any(b.get_replica(0)[0] != np.asarray(cfg4["com"]), axis=1))[0]
        assert moved.size >= 4
        sel = np.concatenate([moved[:4], SEL8[:4]])
        check_selected(orc, cfg4, b, sel, "latency")


def test_after_eval_and_settle(cfg4, orc):
    """Caller proposals with the host's decisions, one of them accepted: the committed S(k) is in
    the other buffer (s_cur = 1) for every replica; the moved molecule is among the selected."""
    a = cfg4
    R = 2
    com, coords = np.asarray(a["com"]), np.asarray(a["coords"])
    with make_batch(a, R) as b:
        d = np.array([0.2, -0.1, 0.15])
        b.eval(np.full(R, 5), np.tile(com[4] + d, (R, 1)), np.tile(coords[12:15] + d, (R, 1, 1)))
        b.eval(np.full(R, 9), np.tile(com[8] - d, (R, 1)), np.tile(coords[24:27] - d, (R, 1, 1)),
               accept_prev=np.ones(R, dtype=bool))
        b.settle(np.zeros(R, dtype=np.int32))
        c1, x1, _ = b.get_replica(1)
        assert np.array_equal(c1[4], com[4] + d) and np.array_equal(c1[8], com[8])
        check_selected(orc, a, b, np.array([4, 8, 0, 63, 64, 301, 700, 749]), "eval/settle")


def test_volume_trial_accept_and_reject(cfg4, orc):
    """One replica: between mmc_batch_volume_trial and its decision the call is refused and writes
    nothing; after a reject the same call gives the same bytes as before the trial; after an accept
    the terms in the new box (get_boxes, kappa = 5.6 / box)."""
    from metropolismontecarlo_amd import _lib
    a = cfg4
    L1 = (1.01 * a["box"] ** 3) ** (1 / 3)
    with make_batch(a, 1) as b:
        b.set_option("device_moves", 1)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        b.run(80, T, 0.3, 0.2, seed=9, energies=e, n_groups=1)
        before = b.deletion(T, sel=SEL8, details=True)
        for accept in (False, True):
            b.volume_trial(L1, 5.6 / L1)
            bs, nf = np.full(1, 7.5), np.full(1, 3, dtype=np.int64)
            with pytest.raises(_lib.MMCError) as ei:
                b.deletion(T, boltz_sum=bs, n_flagged=nf)
            assert ei.value.status == _lib.MMC_ERR_STATE and bs[0] == 7.5 and nf[0] == 3
            if accept:
                b.volume_accept()
            else:
                b.volume_reject()
                again = b.deletion(T, sel=SEL8, details=True)
                for k in before:
                    assert before[k].tobytes() == again[k].tobytes(), k
        assert b.get_boxes()[0] == L1
        check_selected(orc, a, b, SEL8, "volume accept")


def test_after_set_replica_and_recip_long(cfg4, orc):
    """mmc_batch_set_replica on one replica of three, then mmc_batch_recip_long."""
    a = cfg4
    L = float(a["box"])
    com, coords = np.asarray(a["com"]), np.asarray(a["coords"])
    with make_batch(a, 3) as b:
        shift = np.array([1.3, -2.1, 0.4])
        c2 = (com + shift) % L
        x2 = coords + np.repeat(c2 - com, 3, axis=0)
        c2[10] += np.array([0.3, 0.2, -0.1])
        x2[30:33] += np.array([0.3, 0.2, -0.1])
        b.set_replica(1, c2, x2)
        b.recip_long()
        assert np.array_equal(b.get_replica(1)[0], c2)
        check_selected(orc, a, b, np.array([10, 0, 63, 64, 301, 511, 700, 749]), "set_replica")
