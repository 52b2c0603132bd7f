"""Virtual volume moves (mmc_batch_volume_perturb) on the rest of what its three kernels read or
branch on, against the oracle (test_gpu_volume_perturb.py has the definition, the sums and the
refusals):
  1. launches in chunks of replicas (va.r0, the chunk-local index of the partials);
  2. the series below r^2 = 0.25, the one place where k_vp_pairs takes the test box's kappa itself;
  3. odd atom counts (k_vp_recip's S(k) offset) and 6. the tile shapes: one tile, N below, at and
     above multiples of 64, the largest system the LDS rule accepts and the refusal beyond it;
  4. separate LJ and Coulomb cutoffs (the two gate bits);
  5. nine LJ pairs per molecule pair;
  7. where an overlap sits: tile, scale index, and one that is there already at f = 1;
  8. one and eight test boxes;
  9. the committed state (records, coordinates, box, kappa) after every path that changes it --
     the cases of tests/test_gpu_deletion_paths.py;
 10. volume changes dv converted with the batch's CURRENT box.
Every comparison is part by part on get_replica's configuration in the box of get_boxes(), with the
measure and tolerance of test_gpu_volume_perturb.py (rel(x, ref, 1.0) < 1e-9), flags exact.  The
CPU side of every input (table domain, constructions) is tests/test_volume_perturb_host.py."""
import re

import numpy as np
import pytest

import common
import volume_perturb_ref as ref
from common import rel
from test_gpu_volume_perturb import DPHI, DR, TOL, W_TOL, check_against_oracle, raw_call
from test_volume_perturb_host import (ALPHA, CHUNK_N, CHUNK_SCALES, CONTACT_PAIR, CONTACT_R2, CUTOFFS, EDGE_RCUT,
                                      EDGE_SCALES, EIGHT_SCALES, LARGE_RCUT, LARGE_SCALES, LJ9_RCUT, LJ9_SCALES,
                                      MID_OVL_SCALES, NPT_SCALES, OVL_NOW_R2, OVL_PAIRS, PREFIX_N, RCUT, T)
from metropolismontecarlo_amd import _lib, structs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def cfg1():
    return common.nist_arrays(1, "unwrapped")


def make_batch(a, R, lj=EDGE_RCUT, qq=None, steps=0, seed=11):
    """R replicas of `a`, S(k) built; with steps > 0 every replica runs that many trial moves of its
    own stream (default options), so that the replicas are in distinct states."""
    from metropolismontecarlo_amd.device import Batch
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
              ALPHA / a["box"], structs.factor, lj, lj if qq is None else qq)
    b.recip_long()
    if steps:
        e0 = b.potential_ewald(as_array=True)["energy"].copy()
        b.run(steps, T, DR, DPHI, seed=seed, energies=e0)
    return b


def check(orc, a, b, scales, lj, qq=None, replicas=None, what="", out=None):
    """check_against_oracle of test_gpu_volume_perturb.py for the cases it does not take: two cutoffs,
    a box that has changed (get_boxes(), kappa = alpha / box), overlaps -- where the flags, the zero
    weight and the +inf real part must be the oracle's, and every other part still its number."""
    qq = lj if qq is None else qq
    box = float(b.get_boxes()[0])
    assert ref.domain_ok(box, max(lj, qq), scales, ALPHA), (what, box)   # a refusal would be the test's fault
    bs, no, du, base = b.volume_perturb(T, scales, details=True) if out is None else out
    K = len(scales)
    assert bs.shape == (b.R, K) and no.shape == (b.R, K) and du.shape == (b.R, K, 4) and base.shape == (b.R, 4)
    for r in (range(b.R) if replicas is None else replicas):
        com, coords, _ = b.get_replica(r)
        want = ref.perturb(orc, dict(a, com=com, coords=coords, box=box), scales, ALPHA / box, lj, T, qq_rcut=qq)
        for c, name in enumerate(ref.PARTS):
            if c == 1 and want["ovl0"]:
                assert base[r, 1] == np.inf, (what, r)
            else:
                print(what, r, name, base[r, c], want["base"][c])
                assert rel(base[r, c], want["base"][c], 1.0) < TOL, (what, r, name, base[r, c], want["base"][c])
        for k in range(K):
            assert no[r, k] == int(want["ovl"][k]), (what, r, k)
            for c, name in enumerate(ref.PARTS):
                if c == 1 and want["ovl"][k]:
                    assert du[r, k, 1] == np.inf and bs[r, k] == 0.0, (what, r, k)
                    continue
                got, exp = base[r, c] + du[r, k, c], want["base"][c] + want["du"][k, c]
                print(what, r, k, name, got, exp)
                assert rel(got, exp, 1.0) < TOL, (what, r, k, name, got, exp)
        fin = ~want["ovl"]                                       # (forced weights are 0.0, asserted above)
        w, _ = ref.weights(du[r][fin], fin[fin] & False, np.asarray(scales)[fin], b.n_mol, T)
        with np.errstate(invalid="ignore"):                     # (a weight may overflow to +inf on both sides)
            assert np.all((bs[r][fin] == w) | (np.abs(bs[r][fin] - w) <= W_TOL * np.abs(w))), (what, r, bs[r], w)
    for k, f in enumerate(scales):
        if f == 1.0:                                            # exactly zero, weight exactly one
            ok = no[:, k] == 0
            assert np.array_equal(du[ok, k], np.zeros((int(ok.sum()), 4))), what
            assert np.array_equal(bs[ok, k], np.ones(int(ok.sum()))), what
    return bs, no, du, base


def same_rows(x, y, rows):
    """The outputs of two calls hold the same bytes in these replicas' rows."""
    return all(u[r].tobytes() == v[r].tobytes() for u, v in zip(x, y) for r in rows)


# ---- 1. chunks ----------------------------------------------------------------------------------
def test_replicas_beyond_the_first_chunk(orc, cfg1):
    """32768 + 5 replicas of 16 molecules (one tile pair) and one test box: the chunk is the cap of
    32768 replicas, so the second launch starts at r0 = 32768 with five replicas.  Replicas 0, 32767,
    32768, 32769 and R - 1 hold five configurations of their own (set_replica), all others the
    construction state: the five against the oracle, three untouched ones -- one of the first chunk,
    two of the second, hence five replicas there and not three -- bit-equal to each other and to
    none of the five, and a second call accumulating into the first call's sums.
    The other chunk size, the 256 MiB bound on the partials, needs about 16 000 replicas of 750
    molecules and is deliberately left out."""
    a = ref.prefix(cfg1, CHUNK_N)
    R = 32768 + 5
    touched, plain = (0, 32767, 32768, 32769, R - 1), (5, 32770, 32771)
    states = ref.shifted_states(a, len(touched))
    with make_batch(a, R) as b:
        for r, s in zip(touched, states):
            b.set_replica(r, s["com"], s["coords"])
        b.recip_long()
        out = b.volume_perturb(T, CHUNK_SCALES, details=True)
        bs, no, du, base = check(orc, a, b, CHUNK_SCALES, EDGE_RCUT, replicas=touched + plain[:1], what="chunks", out=out)
        for r in plain[1:]:
            assert all(x[r].tobytes() == x[plain[0]].tobytes() for x in out), r
        for r in touched:
            assert du[r].tobytes() != du[plain[0]].tobytes(), r
        assert len({du[r].tobytes() for r in touched}) == len(touched)
        assert not no.any()
        # every untouched replica, both chunks: the same bytes
        rest = np.setdiff1d(np.arange(R), touched)
        assert np.all(du[rest] == du[plain[0]]) and np.all(base[rest] == base[plain[0]]) and np.all(bs[rest] == bs[plain[0]])
        first = bs.copy()
        bs2, no2 = b.volume_perturb(T, CHUNK_SCALES, boltz_sum=bs, n_overlap=no)
        assert bs2 is bs and no2 is no and not no.any()
        sel = list(touched + plain)
        zero = np.zeros((len(sel), 1), dtype=bool)
        h1, n1 = ref.host_sums(du[sel], zero, CHUNK_SCALES, b.n_mol, T, np.zeros((len(sel), 1)), np.zeros((len(sel), 1)))
        h2, n2 = ref.host_sums(du[sel], zero, CHUNK_SCALES, b.n_mol, T, h1, n1)
        assert np.all(np.abs(first[sel] - h1) <= W_TOL * np.abs(h1))
        assert np.all(np.abs(bs[sel] - h2) <= (W_TOL + 1e-15) * np.abs(h2)) and not n2.any()
        assert np.array_equal(bs, first + first)                # the same weights, added once more


# ---- 2. the series branch -----------------------------------------------------------------------
def test_close_like_charge_contact_takes_the_test_boxes_kappa(orc, cfg1):
    """Two hydrogens at r^2 = 0.2 in replica 1 of three (test_volume_perturb_host.py asserts the
    construction and that the batch's kappa in place of kappa_k would move the real part by 1e-4)."""
    bad, _ = ref.contact_case(cfg1, *CONTACT_PAIR, r2=CONTACT_R2)
    with make_batch(cfg1, 3) as b:
        clean = b.volume_perturb(T, EDGE_SCALES, details=True)
        b.set_replica(1, bad["com"], bad["coords"])
        b.recip_long()
        out = check(orc, cfg1, b, EDGE_SCALES, EDGE_RCUT, what="contact")
        assert not out[1].any() and np.all(np.isfinite(out[2]))
        assert same_rows(out, clean, (0, 2)) and out[2][1].tobytes() != clean[2][1].tobytes()


# ---- 3. and 6. molecule counts ------------------------------------------------------------------
@pytest.mark.parametrize("n_mol", PREFIX_N)
def test_odd_and_edge_molecule_counts(orc, n_mol):
    """Prefixes of a dense water lattice in a fixed 20.85 A box: one tile with one or two molecules
    (no pair, one pair), 63 / 64 / 65 and 128 / 129 molecules (a full tile, a second tile of one
    molecule, three tiles), odd atom counts at every odd N.  Two replicas a few moves apart."""
    a = ref.dense_prefix(n_mol)
    with make_batch(a, 2, steps=12) as b:
        assert not np.array_equal(b.get_replica(0)[0], b.get_replica(1)[0])
        st, untouched = raw_call(b, EDGE_SCALES)
        if n_mol <= 2 and st != _lib.MMC_OK:                    # "a system the table kernels refuse"
            assert st == _lib.MMC_ERR_UNSUPPORTED and untouched, (st, _lib.lib().mmc_last_error())
            return
        assert st == _lib.MMC_OK, (st, _lib.lib().mmc_last_error())
        check(orc, a, b, EDGE_SCALES, EDGE_RCUT, what=n_mol)


@pytest.fixture(scope="module")
def lds_atoms():
    """The atom bound of k_vp_recip's LDS rule, from the refusal of a system far beyond it."""
    from test_gpu_batch import _dense_water
    a = _dense_water(1200)
    with make_batch(a, 1, lj=LARGE_RCUT) as b:
        with pytest.raises(_lib.MMCError) as e:
            b.volume_perturb(T, LARGE_SCALES)
    assert e.value.status == _lib.MMC_ERR_UNSUPPORTED
    m = re.search(r"at most (\d+) atoms", str(e.value))
    assert m, str(e.value)
    return int(m.group(1))


def test_the_largest_system_the_lds_rule_accepts(orc, lds_atoms):
    from test_gpu_batch import _dense_water
    n_mol = lds_atoms // 3
    assert 300 <= n_mol < 1200
    a = _dense_water(n_mol)
    with make_batch(a, 1, lj=LARGE_RCUT, steps=20) as b:
        check(orc, a, b, LARGE_SCALES, LARGE_RCUT, what=("largest", n_mol))


def test_one_molecule_beyond_the_lds_rule_is_refused(lds_atoms):
    from test_gpu_batch import _dense_water
    n_mol = lds_atoms // 3 + 1
    a = _dense_water(n_mol)
    assert ref.domain_ok(a["box"], LARGE_RCUT, LARGE_SCALES, ALPHA)     # the LDS rule alone refuses
    with make_batch(a, 1, lj=LARGE_RCUT) as b:
        st, untouched = raw_call(b, LARGE_SCALES)
        assert st == _lib.MMC_ERR_UNSUPPORTED and untouched, (st, _lib.lib().mmc_last_error())
        assert f"at most {lds_atoms} atoms" in _lib.lib().mmc_last_error().decode()


# ---- 4. separate cutoffs ------------------------------------------------------------------------
@pytest.mark.parametrize("config,lj,qq,scales", CUTOFFS)
def test_separate_cutoffs(orc, config, lj, qq, scales):
    a = common.nist_arrays(config, "unwrapped")
    with make_batch(a, 2, lj=lj, qq=qq, steps=30) as b:
        check(orc, a, b, scales, lj, qq, what=(config, lj, qq))


# ---- 5. nine LJ pairs ---------------------------------------------------------------------------
def test_nine_lj_pairs_per_molecule_pair(orc):
    a = ref.lj9_system()
    with make_batch(a, 2, lj=LJ9_RCUT, steps=30) as b:
        assert not np.array_equal(b.get_replica(0)[0], b.get_replica(1)[0])
        check(orc, a, b, LJ9_SCALES, LJ9_RCUT, what="lj9")


# ---- 7. where an overlap sits -------------------------------------------------------------------
@pytest.mark.parametrize("where", sorted(OVL_PAIRS))
def test_overlap_positions(orc, cfg1, where):
    """An O-H pair at r^2 = 0.52 inside tile 0, across the two tiles and inside the ragged last tile,
    in replica 1 of three; the compressing scale is third of four."""
    bad, _ = ref.overlap_case(cfg1, *OVL_PAIRS[where])
    with make_batch(cfg1, 3) as b:
        clean = b.volume_perturb(T, MID_OVL_SCALES, details=True)
        b.set_replica(1, bad["com"], bad["coords"])
        out = check(orc, cfg1, b, MID_OVL_SCALES, EDGE_RCUT, what=where)
        bs, no, du, base = out
        assert np.array_equal(no, [[0] * 4, [0, 0, 1, 0], [0] * 4])
        assert bs[1, 2] == 0.0 and du[1, 2, 1] == np.inf and bs[1, 1] == 1.0
        assert np.all(np.isfinite(base)) and np.all(np.isfinite(du[1, [0, 1, 3]]))
        assert same_rows(out, clean, (0, 2))


def test_overlap_already_there_at_scale_one(orc, cfg1):
    bad, _ = ref.overlap_case(cfg1, 0, 1, r2=OVL_NOW_R2)
    with make_batch(cfg1, 3) as b:
        clean = b.volume_perturb(T, MID_OVL_SCALES, details=True)
        b.set_replica(1, bad["com"], bad["coords"])
        out = check(orc, cfg1, b, MID_OVL_SCALES, EDGE_RCUT, what="stored overlap")
        bs, no, du, base = out
        assert np.array_equal(no, [[0] * 4, [1] * 4, [0] * 4]) and np.all(bs[1] == 0.0)
        assert base[1, 1] == np.inf and np.all(du[1, :, 1] == np.inf)
        assert np.all(np.isfinite(base[1, [0, 2, 3]])) and np.all(np.isfinite(du[1][:, [0, 2, 3]]))
        assert same_rows(out, clean, (0, 2))


# ---- 8. one and eight test boxes ----------------------------------------------------------------
def test_eight_scales_equal_eight_calls_of_one(orc, cfg1):
    with make_batch(cfg1, 3, steps=30) as b:
        bs, no, du, base = check_against_oracle(orc, cfg1, b, EIGHT_SCALES, EDGE_RCUT, what="eight")
        for k, f in enumerate(EIGHT_SCALES):
            b1, n1, d1, base1 = b.volume_perturb(T, [f], details=True)
            assert b1.shape == (3, 1) and d1.shape == (3, 1, 4)
            assert d1[:, 0].tobytes() == np.ascontiguousarray(du[:, k]).tobytes(), k
            assert b1[:, 0].tobytes() == np.ascontiguousarray(bs[:, k]).tobytes(), k
            assert base1.tobytes() == base.tobytes() and not n1.any(), k


# ---- 9. after every path that changes the committed state ---------------------------------------
def test_after_host_decided_runs(orc, cfg1):
    """One step per launch, the host decides (persistent = 0, accept_on_device = 0)."""
    with make_batch(cfg1, 8) as b:
        for k, v in (("device_moves", 1), ("kernel", 2), ("persistent", 0), ("accept_on_device", 0)):
            b.set_option(k, v)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        e, st = b.run(37, T, 0.3, 0.2, seed=5, energies=e)
        assert st["device_decisions"] == 0 and st["trans_accept"] + st["rot_accept"] > 0
        check(orc, cfg1, b, EDGE_SCALES, EDGE_RCUT, replicas=(0, 3, 4, 7), what="host-decided")


def test_after_kernel_decided_runs(orc, cfg1):
    """Eight steps per launch, the kernel decides, 24 replicas in two groups on one workgroup; the
    chains go on bit for bit like a twin's that made no such call."""
    R, per_launch = 24, 8
    opts = (("device_moves", 1), ("kernel", 2), ("persistent", 0), ("accept_on_device", 1),
            ("steps_per_launch", per_launch), ("wave_wgs", 1))
    with make_batch(cfg1, R) as b, make_batch(cfg1, R) as tw:
        es = []
        for x in (b, tw):
            for k, v in opts:
                x.set_option(k, v)
            e = x.potential_ewald(as_array=True)["energy"].copy()
            e, st = x.run(3 * per_launch + 5, T, 0.3, 0.2, seed=6, energies=e, n_groups=2, n_parts=1)
            assert st["device_decisions"] == R * (3 * per_launch + 5)
            es.append(e)
        check(orc, cfg1, b, EDGE_SCALES, EDGE_RCUT, replicas=(0, 11, 12, 23), what=per_launch)
        for x, k in ((b, 0), (tw, 1)):
            es[k], _ = x.run(2 * per_launch + 3, T, 0.3, 0.2, seed=7, energies=es[k], n_groups=2, n_parts=1)
        assert es[0].tobytes() == es[1].tobytes()
        for r in range(R):
            for u, v in zip(b.get_replica(r), tw.get_replica(r)):
                assert np.asarray(u).tobytes() == np.asarray(v).tobytes(), r


def test_after_the_latency_server(orc):
    """One replica of 750 molecules with the default options: the latency server runs the chain."""
    a = common.nist_arrays(4, "unwrapped")
    with make_batch(a, 1, lj=RCUT) as b:
        b.set_option("device_moves", 1)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        e, st = b.run(150, T, 0.3, 0.2, seed=8, energies=e, n_groups=1)
        assert st["server_steps"] == 150 and st["trans_accept"] + st["rot_accept"] > 0
        check(orc, a, b, NPT_SCALES, RCUT, what="latency")


def test_after_eval_and_settle(orc, cfg1):
    """Caller proposals with the host's decisions, one of them accepted."""
    a, R = cfg1, 2
    com, coords = np.asarray(a["com"]), np.asarray(a["coords"])
    with make_batch(a, R) as b:
        d = np.array([0.2, -0.1, 0.15])
        b.eval(np.full(R, 5), np.tile(com[4] + d, (R, 1)), np.tile(coords[12:15] + d, (R, 1, 1)))
        b.eval(np.full(R, 9), np.tile(com[8] - d, (R, 1)), np.tile(coords[24:27] - d, (R, 1, 1)),
               accept_prev=np.ones(R, dtype=bool))
        b.settle(np.zeros(R, dtype=np.int32))
        c1, x1, _ = b.get_replica(1)
        assert np.array_equal(c1[4], com[4] + d) and np.array_equal(c1[8], com[8])
        check(orc, a, b, EDGE_SCALES, EDGE_RCUT, what="eval/settle")


def test_after_set_replica_and_recip_long(orc, cfg1):
    a = cfg1
    s = ref.shifted_states(a, 1)[0]
    with make_batch(a, 3) as b:
        b.set_replica(1, s["com"], s["coords"])
        b.recip_long()
        assert np.array_equal(b.get_replica(1)[0], s["com"])
        out = check(orc, a, b, EDGE_SCALES, EDGE_RCUT, what="set_replica")
        assert out[2][0].tobytes() == out[2][2].tobytes() != out[2][1].tobytes()


def test_volume_trial_accept_and_reject(orc, cfg1):
    """One replica: between mmc_batch_volume_trial and its decision the call is refused and writes
    nothing; after a reject it gives the same bytes as before the trial; after an accept the parts
    in the new box, with the new kappa and the rescaled records."""
    a = cfg1
    L1 = (1.01 * a["box"] ** 3) ** (1 / 3)
    with make_batch(a, 1) as b:
        b.set_option("device_moves", 1)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        b.run(80, T, 0.3, 0.2, seed=9, energies=e, n_groups=1)
        before = b.volume_perturb(T, EDGE_SCALES, details=True)
        for accept in (False, True):
            b.volume_trial(L1, ALPHA / L1)
            st, untouched = raw_call(b, EDGE_SCALES)
            assert st == _lib.MMC_ERR_STATE and untouched
            if accept:
                b.volume_accept()
            else:
                b.volume_reject()
                assert same_rows(before, b.volume_perturb(T, EDGE_SCALES, details=True), (0,))
        assert b.get_boxes()[0] == L1
        out = check(orc, a, b, EDGE_SCALES, EDGE_RCUT, what="volume accept")
        assert out[3].tobytes() != before[3].tobytes()


def npt_chain(b, box0, seed):
    """A few NPT sweeps with at least one accepted volume move."""
    e0 = float(b.potential_ewald(as_array=True)["energy"][0])
    e1, st, ns = b.run_npt(8, T, 0.03, 0.03 * box0 ** 3, 0.3, 0.2, seed, e0, moves_per_sweep=40, alpha=ALPHA)
    assert ns["vol_attempt"] == 8 and ns["vol_accept"] >= 1, ns
    assert b.get_boxes()[0] == ns["box"] != box0
    return ns


def test_after_run_npt(orc, cfg1):
    a = cfg1
    with make_batch(a, 1) as b:
        b.set_option("device_moves", 1)
        ns = npt_chain(b, a["box"], 13)
        check(orc, a, b, NPT_SCALES, EDGE_RCUT, what=("npt", ns["box"], ns["vol_accept"]))


# ---- 10. dv with the current box ----------------------------------------------------------------
def test_dv_is_converted_with_the_current_box(cfg1):
    """Batch.volume_perturb(dv=...) after volume_change, an accepted volume_trial and run_npt: the
    bytes of the call with scale_of_dv(get_boxes()[0], dv); Batch.box and Batch.kappa follow the
    library's box and alpha / box, and a reject puts the old ones back."""
    a = cfg1
    L0, dvs = a["box"], [-60.0, 60.0]

    def dv_equals_scales(what):
        box = float(b.get_boxes()[0])
        sc = [ref.scale_of_dv(box, dv) for dv in dvs]
        assert box == L0 or sc != [ref.scale_of_dv(L0, dv) for dv in dvs]
        assert ref.domain_ok(box, EDGE_RCUT, sc, ALPHA)
        x, y = b.volume_perturb(T, dv=dvs, details=True), b.volume_perturb(T, scales=sc, details=True)
        assert same_rows(x, y, (0,)), what
        assert np.all(x[2][0] != 0.0)
        assert b.box == box and b.kappa == ALPHA / box, (what, b.box, box, b.kappa)

    with make_batch(a, 1) as b:
        b.set_option("device_moves", 1)
        dv_equals_scales("construction")
        L1 = (1.02 * L0 ** 3) ** (1 / 3)
        b.volume_trial(L1, ALPHA / L1)
        assert b.box == L1 and b.kappa == ALPHA / L1
        b.volume_reject()
        assert b.box == L0 and b.kappa == ALPHA / L0
        dv_equals_scales("reject")
        b.volume_trial(L1, ALPHA / L1)
        b.volume_accept()
        assert b.get_boxes()[0] == L1
        dv_equals_scales("accept")
        L2 = (0.99 * L0 ** 3) ** (1 / 3)
        b.volume_change(L2, ALPHA / L2)
        b.recip_long()
        assert b.get_boxes()[0] == L2
        dv_equals_scales("volume_change")
        npt_chain(b, L2, 17)
        dv_equals_scales("run_npt")
