"""mmc_batch_volume_perturb against its restatement on the oracle (tests/volume_perturb_ref.py),
against the state-changing route it replaces (set_boxes, volume_trial_replicas, volume_settle), and
its promises: read-only, reproducible, accumulating, loud.

Energies are compared part by part with the project's TOL = 1e-9 in the relative measure of
tests/test_gpu_npt_replicas.py (rel(x, ref, 1.0): relative, absolute below 1 K)."""
import ctypes as C

import numpy as np
import pytest

import common
import volume_perturb_ref as ref
from common import rel
from test_volume_perturb_host import (ALPHA, EDGE_RCUT, EDGE_SCALES, OVL_SCALES, RCUT, SCALES, T)
from metropolismontecarlo_amd import _lib, structs

pytestmark = pytest.mark.gpu
TOL = 1e-9
DR, DPHI = 0.316555789, 0.05
# a weight recomputed on the host from the call's own dU: the same IEEE operations up to the last
# place of log (times N <= 750: 1e-14 in the argument) and of exp
W_TOL = 1e-13


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def make_batch(a, R, rcut=RCUT, steps=0, seed=11):
    """R replicas of `a`; with steps > 0 every replica runs that many trial moves of its own stream,
    so that the replicas are in distinct states."""
    from metropolismontecarlo_amd.device import Batch
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
              ALPHA / a["box"], structs.factor, rcut, rcut)
    b.recip_long()
    if steps:
        e0 = b.potential_ewald(as_array=True)["energy"].copy()
        b.run(steps, T, DR, DPHI, seed=seed, energies=e0)
    return b


def state(a, b, r):
    com, coords, _ = b.get_replica(r)
    return dict(a, com=com, coords=coords)


def check_against_oracle(orc, a, b, scales, rcut, replicas=None, what=""):
    bs, no, du, base = b.volume_perturb(T, scales, details=True)
    assert bs.shape == (b.R, len(scales)) and du.shape == (b.R, len(scales), 4) and base.shape == (b.R, 4)
    for r in (range(b.R) if replicas is None else replicas):
        want = ref.perturb(orc, state(a, b, r), scales, b.kappa, rcut, T)
        assert not want["ovl"].any()
        for c, name in enumerate(ref.PARTS):
            assert rel(base[r, c], want["base"][c], 1.0) < TOL, (what, r, name, base[r, c], want["base"][c])
            for k in range(len(scales)):
                got, exp = base[r, c] + du[r, k, c], want["base"][c] + want["du"][k, c]
                assert rel(got, exp, 1.0) < TOL, (what, r, k, name, got, exp)
        assert not no[r].any()
    for k, f in enumerate(scales):
        if f == 1.0:                                            # exactly zero, weight exactly one
            assert np.array_equal(du[:, k], np.zeros((b.R, 4))), what
            assert np.array_equal(bs[:, k], np.ones(b.R)), what
    return bs, no, du, base


@pytest.mark.parametrize("variant", ["unwrapped", "reference"])
def test_oracle_parity_three_replicas(orc, variant):
    """750 molecules (12 tiles of 64, the last with 46), whole and broken molecules, three replicas
    in distinct states."""
    a = common.nist_arrays(4, variant)
    with make_batch(a, 3, steps=40) as b:
        assert not np.array_equal(b.get_replica(1)[0], b.get_replica(2)[0])
        check_against_oracle(orc, a, b, SCALES, RCUT, what=variant)


@pytest.mark.parametrize("R", [1, 3, 5])
def test_tile_edges_and_replica_counts(orc, R):
    """100 molecules: two tiles, the second with 36; r_cut = 9 in L = 20, so the smallest test box
    (0.95 L = 19) is still >= 2 r_cut and kappa sqrt(r_cut^2 + 100) = 3.97 inside the table."""
    a = common.nist_arrays(1, "unwrapped")
    with make_batch(a, R, rcut=EDGE_RCUT, steps=30) as b:
        check_against_oracle(orc, a, b, EDGE_SCALES, EDGE_RCUT, what=f"R={R}")


def test_equals_the_state_changing_route_and_leaves_the_batch_alone():
    from test_gpu_npt_replicas import per_box_batch
    a = common.nist_arrays(4, "unwrapped")
    with make_batch(a, 3, steps=40) as b:
        R = b.R
        t0 = b.potential_ewald(as_array=True).copy()
        e0 = b.recip_long().copy()                             # (S(k) rebuilt from the coordinates)
        before = [b.get_replica(r) for r in range(R)]
        bs, no, du, base = b.volume_perturb(T, SCALES, details=True)
        after = [b.get_replica(r) for r in range(R)]
        for r in range(R):
            assert all(np.array_equal(x, y) for x, y in zip(before[r], after[r])), r
        assert np.array_equal(b.recip_long(), e0)
        assert b.potential_ewald(as_array=True).tobytes() == t0.tobytes()
        states = [dict(state(a, b, r), box=a["box"]) for r in range(R)]
        with per_box_batch(states) as twin:
            for k, f in enumerate(SCALES):
                tot = twin.volume_trial_replicas(np.full(R, f * a["box"]))
                twin.volume_settle(np.zeros(R, dtype=np.int32))
                for r in range(R):
                    for c, name in enumerate(ref.PARTS):
                        assert rel(base[r, c] + du[r, k, c], tot[name][r], 1.0) < TOL, (r, k, name)
                    u = base[r].sum() + (((du[r, k, 0] + du[r, k, 1]) + du[r, k, 2]) + du[r, k, 3])
                    assert rel(u, tot["energy"][r], 1.0) < TOL, (r, k)


def test_chains_do_not_notice_the_calls():
    a = common.nist_arrays(1, "unwrapped")
    out = []
    for interleave in (True, False):
        with make_batch(a, 3, rcut=EDGE_RCUT) as b:
            e = b.potential_ewald(as_array=True)["energy"].copy()
            for _ in range(4):
                if interleave:
                    b.volume_perturb(T, EDGE_SCALES)
                e, _ = b.run(10, T, DR, DPHI, seed=99, energies=e)
            if interleave:
                b.volume_perturb(T, dv=[-50.0, 50.0])
            out.append((e, [b.get_replica(r) for r in range(3)]))
    assert np.array_equal(out[0][0], out[1][0])
    for r in range(3):
        assert all(np.array_equal(x, y) for x, y in zip(out[0][1][r], out[1][1][r])), r


def test_reproducible_and_accumulating():
    """Bit-identical from call to call and under another "wave_wgs"; two calls add in call order, and
    the sums are the host's own of the returned dU."""
    a = common.nist_arrays(1, "unwrapped")
    with make_batch(a, 3, rcut=EDGE_RCUT, steps=30) as b:
        bs1, no1, du1, base1 = b.volume_perturb(T, EDGE_SCALES, details=True)
        b.set_option("wave_wgs", 7)
        bs2, no2, du2, base2 = b.volume_perturb(T, EDGE_SCALES, details=True)
        b.set_option("wave_wgs", 0)
        for x, y in ((bs1, bs2), (du1, du2), (base1, base2)):
            assert x.tobytes() == y.tobytes()
        # accumulate: a second call, after a few moves, into the first call's sums
        first = bs1.copy()
        e = b.potential_ewald(as_array=True)["energy"].copy()
        b.run(20, T, DR, DPHI, seed=5, energies=e)
        bs3, no3, du3, _ = b.volume_perturb(T, EDGE_SCALES, boltz_sum=bs1, n_overlap=no1, details=True)
        assert bs3 is bs1 and no3 is no1
        assert not np.array_equal(du3, du1)
        zero = np.zeros((3, len(EDGE_SCALES)), dtype=bool)
        h1, n1 = ref.host_sums(du1, zero, EDGE_SCALES, b.n_mol, T, np.zeros_like(first), np.zeros_like(no2))
        h2, n2 = ref.host_sums(du3, zero, EDGE_SCALES, b.n_mol, T, h1, n1)
        assert np.all((first == h1) | (np.abs(first - h1) <= W_TOL * np.abs(h1)))
        assert np.all((bs1 == h2) | (np.abs(bs1 - h2) <= (W_TOL + 1e-15) * np.abs(h2)))
        assert np.array_equal(no1, n2) and not no1.any()
        # ... exactly the first call's sums plus the second call's weights, in that order
        w3 = b.volume_perturb(T, EDGE_SCALES)[0]
        assert np.array_equal(bs1, first + w3)


def test_overlap_at_the_compressed_box_only(orc):
    a = common.nist_arrays(1, "unwrapped")
    bad, _ = ref.overlap_case(a)
    with make_batch(a, 3, rcut=EDGE_RCUT) as b:
        clean = b.volume_perturb(T, OVL_SCALES, details=True)
        b.set_replica(1, bad["com"], bad["coords"])
        bs, no, du, base = b.volume_perturb(T, OVL_SCALES, details=True)
        assert np.array_equal(no, [[0] * 5, [1, 0, 0, 0, 0], [0] * 5])
        assert bs[1, 0] == 0.0 and du[1, 0, 1] == np.inf and np.all(np.isfinite(base))
        for r in (0, 2):                                       # the other replicas: the same bits
            assert bs[r].tobytes() == clean[0][r].tobytes() and du[r].tobytes() == clean[2][r].tobytes()
        want = ref.perturb(orc, bad, OVL_SCALES, b.kappa, EDGE_RCUT, T)
        assert list(want["ovl"]) == [True, False, False, False, False]
        for k in range(1, 5):                                  # the other test boxes of that replica
            for c, name in enumerate(ref.PARTS):
                got, exp = base[1, c] + du[1, k, c], want["base"][c] + want["du"][k, c]
                assert rel(got, exp, 1.0) < TOL, (k, name, got, exp)
        assert bs[1, 2] == 1.0


def raw_call(b, scales):
    """The C call with sentinel-filled outputs: (status, outputs untouched)."""
    K, R = len(scales), b.R
    sc = np.array(scales, dtype=np.float64)
    bs, du, base = np.full((R, K), 7.5), np.full((R, K, 4), 7.5), np.full((R, 4), 7.5)
    no = np.full((R, K), 77, dtype=np.int64)
    dp = C.POINTER(C.c_double)
    st = b._L.mmc_batch_volume_perturb(b._h, K, sc.ctypes.data_as(dp), T, bs.ctypes.data_as(dp),
                                       no.ctypes.data_as(C.POINTER(C.c_int64)), du.ctypes.data_as(dp),
                                       base.ctypes.data_as(dp))
    return st, bool(np.all(bs == 7.5) and np.all(du == 7.5) and np.all(base == 7.5) and np.all(no == 77))


@pytest.mark.parametrize("case,status", [("boxes", "MMC_ERR_UNSUPPORTED"), ("wolf", "MMC_ERR_UNSUPPORTED"),
                                         ("proposals", "MMC_ERR_STATE"), ("volume_trial", "MMC_ERR_STATE"),
                                         ("small_box", "MMC_ERR_ARG")])
def test_refusals_leave_the_outputs_untouched(case, status):
    a = common.nist_arrays(1, "unwrapped")
    L = a["box"]
    # (per-replica boxes need the table's domain at L = 2 r_cut: r_cut = 10 there, and no compression)
    with make_batch(a, 1, rcut=RCUT if case == "boxes" else EDGE_RCUT) as b:
        scales = (0.99, 1.01)
        if case == "boxes":
            scales = (1.0, 1.01)
            b.set_boxes([L], ALPHA)
        elif case == "wolf":
            b.set_coulomb_style("wolf")
        elif case == "proposals":
            b.eval(3, a["com"][2] + 0.1, a["coords"][6:9] + 0.1)
        elif case == "volume_trial":
            b.volume_trial(1.01 * L, ALPHA / (1.01 * L))
        else:
            scales = (0.99, 0.89)                              # 17.8 < 2 r_cut = 18
        st, untouched = raw_call(b, scales)
        assert st == getattr(_lib, status) and untouched, (st, _lib.lib().mmc_last_error())
        with pytest.raises(_lib.MMCError, match=status):
            b.volume_perturb(T, scales)
        # ... and the call works again once the state is settled
        if case == "proposals":
            b.settle([0])
        elif case == "volume_trial":
            b.volume_reject()
        if case in ("proposals", "volume_trial"):
            st, untouched = raw_call(b, scales)
            assert st == _lib.MMC_OK and not untouched
