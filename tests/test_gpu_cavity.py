"""mmc_batch_cavity / mmc_batch_cavity_at against their numpy restatement (tests/cavity_ref.py).

Every output is an integer or a copy of an fp64 value the header defines bit by bit, so nothing here
has a tolerance: counts, indices and histograms must be equal, nn_r2 and the points bitwise.

Launch shape: k_cavity_lane's unit is a block of 64 probes of one replica (a lane per probe);
workgroup g of G takes the blocks [R B g / G, R B (g + 1) / G) of the replica-major order,
B = ceil(n_probe / 64), and its (up to four) waves share the run's blocks of one replica after the
other.  G is option "wave_wgs", by default at most four workgroups per compute unit."""
import ctypes as C

import numpy as np
import pytest

import cavity_ref as ref
import common
from metropolismontecarlo_amd import _lib, structs
from metropolismontecarlo_amd import observables as obs

pytestmark = pytest.mark.gpu

RCUT = 10.0
T, DR, DPHI = 298.15, 0.3, 0.2
ALPHA = 5.6
RADII8 = (0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 7.0, 11.0)


def make_batch(a, R, rcut=RCUT):
    from metropolismontecarlo_amd.device import Batch
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
              ALPHA / a["box"], structs.factor, rcut, rcut)
    b.recip_long()
    return b


def same_bytes(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def run_call(b, points, probes, **kw):
    """cavity(*probes) or cavity_at(points)."""
    if points is None:
        n_probe, seed, draw0 = probes
        return b.cavity(n_probe, seed, draw0, **kw)
    return b.cavity_at(points, **kw)


def check_batch(b, boxes, radii, n_cap, site=0, nn_bins=0, nn_max=None, points=None, probes=(64, 1, 0),
                replicas=None, again=True, what=""):
    """One detailed per-replica call and one summed call against the restatement of every replica in
    `replicas` (default all) and against each other.  Returns (per, tot, [restatement per replica])."""
    R = b.R
    kw = dict(radii=radii, site=site, n_cap=n_cap, nn_bins=nn_bins, nn_max=nn_max)
    per = run_call(b, points, probes, per_replica=True, details=True, **kw)
    tot = run_call(b, points, probes, **kw)
    K, P = len(radii), per["points"].shape[1]
    assert per["occ_hist"].shape == (R, K, n_cap + 1) and tot["occ_hist"].shape == (K, n_cap + 1)
    assert per["occ_mom"].shape == (R, K, 2) and tot["occ_mom"].shape == (K, 2)
    assert per["count"].shape == (R, P, K) and per["nn_r2"].shape == (R, P) and per["nn_idx"].shape == (R, P)
    assert ("nn_hist" in per) == (nn_bins > 0)
    wants = {}
    for r in (range(R) if replicas is None else replicas):
        com, coords, _ = b.get_replica(r)
        want = ref.cavity(ref.sites_of(com, coords, site), per["points"][r], float(boxes[r]), radii, n_cap,
                          nn_bins, nn_max)
        wants[r] = want
        assert np.array_equal(per["count"][r], want["count"]), (what, r)
        assert np.array_equal(per["nn_idx"][r], want["nn_idx"]), (what, r)
        assert same_bytes(per["nn_r2"][r], want["nn_r2"]), (what, r)
        assert np.array_equal(per["occ_hist"][r], want["occ_hist"]), (what, r)
        assert np.array_equal(per["occ_mom"][r], want["occ_mom"]), (what, r)
        if nn_bins > 0:
            assert np.array_equal(per["nn_hist"][r], want["nn_hist"]), (what, r)
    # sum rules, summed outputs, and identical bytes from call to call
    assert np.all(per["occ_hist"].sum(-1) == P), what
    assert np.array_equal(tot["occ_hist"], per["occ_hist"].sum(0)), what
    assert np.array_equal(tot["occ_mom"], per["occ_mom"].sum(0)), what
    if nn_bins > 0:
        assert np.all(per["nn_hist"].sum(-1) == P), what
        assert np.array_equal(tot["nn_hist"], per["nn_hist"].sum(0)), what
    if again:
        rep = run_call(b, points, probes, per_replica=True, details=True, **kw)
        for k in per:
            assert same_bytes(per[k], rep[k]), (what, k)
    return per, tot, wants


# ---- 1. small and odd shapes ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_mol", [1, 2, 63, 64, 65, 129])
def test_small_and_odd_shapes(n_mol):
    """One molecule, two, and the edges of what a staging pass of 64, 128 or 256 threads copies; 1, 63,
    64, 65 and 200 probes are the edges of a 64-probe block: a lone lane, one lane idle, a full wave,
    a second block of one probe, and four blocks (one per wave of the workgroup) with the last part
    filled.  Atom types are mixed, so the SoA arrays are read."""
    box = 22.0
    a = common.random_system(n_mol, box, seed=500 + n_mol)
    with make_batch(a, 3) as b:
        for r in (1, 2):                                       # replicas differ (S(k) is left stale: not read)
            sh = np.random.default_rng(r).random(3) * box
            com = (a["com"] + sh) % box
            b.set_replica(r, com, a["coords"] + np.repeat(com - a["com"], 3, axis=0))
        for n_probe in (1, 63, 64, 65, 200):
            for site in (0, 2, -1):
                what = f"n_mol {n_mol}, {n_probe} probes, site {site}"
                last = n_probe == 200
                check_batch(b, [box] * 3, (3.0,), 1, site, probes=(n_probe, 11 + n_mol, 5), again=last, what=what)
                per, _, wants = check_batch(b, [box] * 3, RADII8, 8, site, nn_bins=33, nn_max=7.5,
                                            probes=(n_probe, 11 + n_mol, 5), again=last, what=what + ", K = 8")
                if n_mol == 129 and last:                      # both ends of the histogram are exercised
                    for r in range(3):
                        assert wants[r]["count"][:, 0].min() == 0 and wants[r]["count"][:, -1].max() > 8
                        assert wants[r]["occ_hist"][0, 0] > 0 and wants[r]["occ_hist"][-1, -1] > 0


# ---- 2. the generator ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cfg4():
    return common.nist_arrays(4, "unwrapped")


def test_generator_is_widoms_and_the_host_mirrors(cfg4):
    from metropolismontecarlo_amd.device import philox4x32
    seed, draw0, M = 0x1234_5678_9abc_def0, (1 << 33) + 7, 200
    with make_batch(cfg4, 4) as b:
        out = b.cavity(M, seed, draw0, details=True)
        pts = out["points"]
        assert pts.shape == (4, M, 3) and np.all((pts >= 0) & (pts < b.box))
        _, _, mol, _, _ = b.widom(M, T, seed=seed, draw0=draw0, outputs=True)
        assert same_bytes(pts, np.ascontiguousarray(mol[..., 9:12]))
        for r in (0, 3):
            assert same_bytes(pts[r], obs.cavity_points(philox4x32, seed, draw0, M, r, b.box)), r
        # draw0 continues the stream: two calls of 100 probes are one call of 200
        first = b.cavity(100, seed, draw0, details=True)
        second = b.cavity(100, seed, draw0 + 100, details=True)
        for k in ("points", "count", "nn_r2", "nn_idx"):
            assert same_bytes(np.concatenate([first[k], second[k]], axis=1), out[k]), k
        for k in ("occ_hist", "occ_mom"):
            assert np.array_equal(first[k] + second[k], out[k]), k
        assert not same_bytes(b.cavity(M, seed + 1, draw0, details=True)["points"], pts)


# ---- 3. adversarial points -------------------------------------------------------------------------------
def test_adversarial_points():
    a = common.nist_arrays(1, "unwrapped")
    L = float(a["box"])
    assert L == 20.0
    coords = np.array(a["coords"], dtype=np.float64).copy()
    # dyadic positions, so that every difference below is exact
    p_tie, v = np.array([4.0, 4.5, 5.0]), np.array([0.125, 0.25, 0.0625])
    coords[3 * 7], coords[3 * 3] = p_tie + v, p_tie - v        # mirror images about the probe
    coords[3 * 11] = (12.5, 7.25, 3.0)                         # L / 2 from a probe along x
    coords[3 * 20] = (15.0, 15.0, 15.0)                        # exactly 3 from a probe
    top = np.nextafter(L, 0.0)
    pts = np.array([coords[3 * 5],                             # 0: on a site
                    p_tie,                                     # 1: two sites at bit-equal r^2
                    (2.5, 7.25, 3.0),                          # 2: |dx| == L / 2 exactly
                    (12.5 - np.nextafter(10.0, 0.0), 7.25, 3.0),   # 3: just under it (one ulp of 10: exact)
                    (0.0, 0.0, 0.0), (top, top, top),          # 4, 5: the ends of [0, L)
                    (12.0, 15.0, 15.0),                        # 6: a site at r^2 == 3.0^2
                    (top, 0.0, 9.5)])
    radii = (0.25, 1.0, 3.0, 10.0)
    with make_batch(a, 2) as b:
        b.set_replica(0, a["com"], coords)                     # replica 1 keeps the fixture
        points = np.stack([pts, pts])
        per, _, wants = check_batch(b, [L, L], radii, 6, nn_bins=7, nn_max=1.0, points=points, what="adversarial")
        w = wants[0]
        r2 = ref.distances2(pts, coords[0::3], L)
        # on a site: r^2 = 0, counted at every radius, bin 0, that site reported
        assert per["nn_r2"][0, 0] == 0.0 and per["nn_idx"][0, 0] == 5 and np.all(per["count"][0, 0] >= 1)
        assert ref.nn_bin(per["nn_r2"][0, :1], 7, 1.0)[0] == 0
        # mirror images: equal bits, the lower index wins
        assert r2[1, 3].tobytes() == r2[1, 7].tobytes() == w["nn_r2"][1].tobytes()
        assert per["nn_idx"][0, 1] == 3
        # |d| == L / 2 and just under it
        assert r2[2, 11] == 100.0 and r2[3, 11] < 100.0
        assert per["count"][0, 2, 3] == (r2[2] < 100.0).sum() and per["count"][0, 3, 3] == (r2[3] < 100.0).sum()
        # strict inequality at r^2 == R^2
        assert r2[6, 20] == 9.0 and per["count"][0, 6, 2] == (r2[6] < 9.0).sum() == (r2[6] <= 9.0).sum() - 1
        # both ends of the nearest-site histogram are used
        assert w["nn_hist"][0] >= 1 and w["nn_hist"][-1] >= 1
        # the other sites, through the COM as well
        check_batch(b, [L, L], radii, 6, site=1, nn_bins=7, nn_max=1.0, points=points, what="adversarial, site 1")
        check_batch(b, [L, L], radii, 6, site=-1, nn_bins=4096, nn_max=L, points=points, what="adversarial, COM")


# ---- 4. launch shape and paths ---------------------------------------------------------------------------
@pytest.mark.parametrize("system", ["records", "arrays"])
def test_launch_shape_and_staging_do_not_change_the_results(system):
    a = common.nist_arrays(1, "unwrapped") if system == "records" else common.random_system(65, 22.0, seed=17, n_types=2)
    R = 5
    with make_batch(a, R) as b:
        rng = np.random.default_rng(5)
        for r in range(1, R):                                  # replicas moved as a whole
            sh = rng.random(3) * a["box"]
            b.set_replica(r, a["com"] + sh, a["coords"] + sh)
        boxes = [a["box"]] * R
        kw = dict(radii=(1.0, 2.5, 4.0, 9.0), n_cap=12, nn_bins=50, nn_max=6.0)
        base_per, base_tot, _ = check_batch(b, boxes, probes=(200, 77, 3), what=system, **kw)
        assert not np.array_equal(base_per["count"][0], base_per["count"][R - 1])
        for wgs, stage in ((1, 1), (7, 1), (0, 0), (1, 0), (7, 0)):
            b.set_option("wave_wgs", wgs)
            b.set_option("local_stage", stage)
            per = b.cavity(200, 77, 3, per_replica=True, details=True, **kw)
            tot = b.cavity(200, 77, 3, **kw)
            for k in base_per:
                assert same_bytes(per[k], base_per[k]), (system, wgs, stage, k)
            for k in base_tot:
                assert same_bytes(tot[k], base_tot[k]), (system, wgs, stage, k)
        b.set_option("wave_wgs", 0)
        b.set_option("local_stage", 1)


def test_a_system_too_large_to_stage():
    """3000 sites are 72 000 bytes of positions: more than the 65 536 of a workgroup."""
    box = 45.0
    a = common.random_system(3000, box, seed=23)
    with make_batch(a, 2) as b:
        sh = np.array([3.25, 7.5, 11.0])
        b.set_replica(1, a["com"] + sh, a["coords"] + sh)
        per, _, wants = check_batch(b, [box] * 2, (1.5, 3.0, 6.0), 40, nn_bins=64, nn_max=4.0, probes=(64, 9, 0),
                                    what="3000 molecules")
        assert wants[0]["count"][:, -1].max() > 20
        check_batch(b, [box] * 2, (1.5, 3.0, 6.0), 40, site=-1, probes=(64, 9, 0), again=False,
                    what="3000 molecules, COM")


# ---- 5. box modes and styles -----------------------------------------------------------------------------
def test_per_replica_boxes():
    from metropolismontecarlo_amd.device import philox4x32
    from test_gpu_local_order import per_box_batch, per_box_states
    states = per_box_states([0.97, 1.0, 1.04])
    with per_box_batch(states) as b:
        boxes = b.get_boxes()
        assert len(set(boxes.tolist())) == 3
        radii = (1.0, 2.0, 3.3, 0.5 * boxes.min())
        per, _, _ = check_batch(b, boxes, radii, 64, nn_bins=100, nn_max=5.0, probes=(100, 31, 2), what="per box")
        for r in range(3):                                     # the points scale with the replica's own box
            assert same_bytes(per["points"][r], obs.cavity_points(philox4x32, 31, 2, 100, r, boxes[r])), r
        check_batch(b, boxes, radii, 64, site=-1, probes=(65, 31, 2), again=False, what="per box, COM")
        with pytest.raises(_lib.MMCError) as ei:
            b.cavity(10, 1, radii=(np.nextafter(0.5 * boxes.min(), 100.0),))
        assert ei.value.status == _lib.MMC_ERR_ARG


def test_wolf_style_returns_the_same_bytes():
    a = common.nist_arrays(1, "unwrapped")
    with make_batch(a, 3) as b:
        b.set_option("device_moves", 1)
        b.run(90, T, 0.4, 0.2, seed=8)
        kw = dict(radii=(1.0, 3.3), n_cap=20, nn_bins=40, nn_max=4.0, per_replica=True, details=True)
        ewald = b.cavity(130, 5, **kw)
        b.set_coulomb_style("wolf")
        wolf = b.cavity(130, 5, **kw)
        for k in ewald:
            assert same_bytes(ewald[k], wolf[k]), k
        check_batch(b, [a["box"]] * 3, (1.0, 3.3), 20, probes=(130, 5, 0), again=False, what="wolf")
        assert not np.array_equal(ewald["count"][0], ewald["count"][1])


# ---- 6. read-only ----------------------------------------------------------------------------------------
def chain(b, interleave, n_blocks=2, steps=60):
    e = b.potential_ewald(as_array=True)["energy"].copy()
    stats = []
    for blk in range(n_blocks):
        e, st = b.run(steps, T, DR, DPHI, seed=21, energies=e)
        stats.append({k: v for k, v in st.items() if isinstance(v, int)})
        if interleave:
            b.cavity(100, 3, 100 * blk, radii=(1.0, 3.3), nn_bins=40, nn_max=5.0, per_replica=bool(blk & 1),
                     details=bool(blk & 1))
            b.cavity_at(np.full((b.R, 3, 3), 1.25), site=-1)
    return e, stats, [b.get_replica(r) for r in range(b.R)]


def test_calls_between_blocks_leave_the_chain_bit_identical():
    """Energies, coordinates and S(k) (get_replica's third array) of 2 x 60 steps with calls after
    each block, against the same chain without."""
    a = common.nist_arrays(1, "unwrapped")
    runs = []
    for interleave in (False, True):
        with make_batch(a, 4) as b:
            b.set_option("device_moves", 1)
            runs.append(chain(b, interleave))
    x, y = runs
    assert x[0].tobytes() == y[0].tobytes()
    assert x[1] == y[1]
    for p, q in zip(x[2], y[2]):
        assert all(u.tobytes() == v.tobytes() for u, v in zip(p, q))


# ---- 7. refusals with a batch ----------------------------------------------------------------------------
def raw_call(b, points=None, n_probe=10, radii=(1.0, 2.0), n_cap=4, nn_bins=16, nn_max=5.0):
    """The C entry points with sentinel outputs.  Returns (status, whether every output is untouched)."""
    R, K = b.R, len(radii)
    rad = np.array(radii, dtype=np.float64)
    out = dict(oh=np.full((K, n_cap + 1), 99, dtype=np.uint64), om=np.full((K, 2), 99, dtype=np.uint64),
               nh=np.full(nn_bins + 1, 99, dtype=np.uint64), pt=np.full((R, n_probe, 3), 7.5),
               ct=np.full((R, n_probe, K), -5, dtype=np.int32), r2=np.full((R, n_probe), 7.5),
               ix=np.full((R, n_probe), -5, dtype=np.int32))
    before = {k: v.copy() for k, v in out.items()}

    def p(k, ct):
        return out[k].ctypes.data_as(C.POINTER(ct))
    common_args = (0, K, rad.ctypes.data_as(C.POINTER(C.c_double)), n_cap, nn_bins, nn_max, 0,
                   p("oh", C.c_uint64), p("om", C.c_uint64), p("nh", C.c_uint64))
    tail = (p("ct", C.c_int32), p("r2", C.c_double), p("ix", C.c_int32))
    L = _lib.lib()
    if points is None:
        st = L.mmc_batch_cavity(b._h, n_probe, 1, 0, *common_args, p("pt", C.c_double), *tail)
    else:
        pts = np.ascontiguousarray(points, dtype=np.float64)
        st = L.mmc_batch_cavity_at(b._h, n_probe, pts.ctypes.data_as(C.POINTER(C.c_double)), *common_args, *tail)
    return st, all(same_bytes(out[k], before[k]) for k in out)


def test_refusals_leave_outputs_untouched():
    a = common.nist_arrays(1, "unwrapped")
    R = 2
    with make_batch(a, R) as b:
        pts = np.full((R, 10, 3), 2.5)
        # a radius above half of the (smallest) box
        for points in (None, pts):
            assert raw_call(b, points, radii=(1.0, np.nextafter(a["box"] / 2, 100.0))) == (_lib.MMC_ERR_ARG, True)
        # a non-finite point
        for bad in (float("nan"), float("inf"), -float("inf")):
            q = pts.copy()
            q[1, 9, 2] = bad
            assert raw_call(b, q) == (_lib.MMC_ERR_ARG, True)
        # proposals outstanding
        com, coords = np.asarray(a["com"]), np.asarray(a["coords"])
        b.eval(np.full(R, 3), np.tile(com[2], (R, 1)), np.tile(coords[6:9], (R, 1, 1)))
        for points in (None, pts):
            assert raw_call(b, points) == (_lib.MMC_ERR_STATE, True)
        b.settle(np.zeros(R, dtype=np.int32))
        # ... and after all that the calls work, a radius of exactly L / 2 included
        for points in (None, pts):
            st, untouched = raw_call(b, points, radii=(1.0, a["box"] / 2))
            assert st == _lib.MMC_OK and not untouched
        assert b.cavity(10, 1, radii=(a["box"] / 2,), n_cap=255)["occ_hist"].sum() == R * 10


# ---- 8. at size ------------------------------------------------------------------------------------------
def test_750_molecules(cfg4):
    nn_bins, nn_max = 400, 5.0
    dr = np.float64(nn_max) / nn_bins
    ms = [40 * k for k in range(1, 9)]                         # 0.5 .. 4.0 in steps of 0.5, built as m * dr
    radii = [m * dr for m in ms]
    assert np.allclose(radii, np.arange(1, 9) * 0.5, rtol=0, atol=1e-12)
    with make_batch(cfg4, 4) as b:
        b.set_option("device_moves", 1)
        b.run(300, T, DR, DPHI, seed=4242)
        per, tot, _ = check_batch(b, [cfg4["box"]] * 4, radii, 32, nn_bins=nn_bins, nn_max=nn_max,
                                  probes=(256, 2024, 0), replicas=(0, 3), what="cfg4")
        assert not np.array_equal(per["count"][0], per["count"][3])
        assert tot["occ_hist"][:, -1].sum() == 0 and tot["occ_hist"][-1, 0] < tot["occ_hist"][0, 0]
        # p0 at the edge m dr from the nearest-site histogram IS the empty bin of the radius m dr
        for h, occ in ((tot["nn_hist"], tot["occ_hist"]), (per["nn_hist"][2], per["occ_hist"][2])):
            tail = np.cumsum(h[::-1])[::-1]
            for k, m in enumerate(ms):
                assert tail[m] == occ[k, 0], (k, m)
        edges, p0 = obs.cavity_size_distribution(tot["nn_hist"], nn_max)
        assert np.array_equal(edges[ms], radii)
        assert np.array_equal(p0[ms] * (4 * 256), tot["occ_hist"][:, 0].astype(np.float64))
        mean, var = obs.occupancy_moments(tot["occ_mom"], 4 * 256)
        rho = 750 / cfg4["box"] ** 3
        assert abs(mean[-1] - rho * 4.0 / 3.0 * np.pi * 64.0) < 1.0 and np.all(var > 0)
