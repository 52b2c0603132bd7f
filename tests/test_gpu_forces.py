"""Forces and torques (mmc_batch_forces) against the numpy restatement of the header's definition
(forces_ref.molecule, pinned on the oracle by central differences in tests/test_forces_host.py),
against mmc_batch_deletion and against the rules the header states.

Tolerance per value: 1e-12 A + 1e-300, A the same sum over the absolute values of its terms
(forces_ref).  The erfc table is within 4e-14 relative (tests/test_gpu_table.py), exp within an ulp
and each term takes a handful of roundings: under 1e-13 of its size, so 1e-12 leaves a factor of ten.
Record of one run on an MI355X: the worst |x - ref| / A over all three shapes was 1.6e-15; the worst
|finite difference of deletion - F| over its allowed error (h = 1e-3 A) was 0.033.

Launch shape: k_forces_wave runs WV_WAVES = 4 waves per workgroup on at most "wave_wgs" workgroups;
unit u is entry u % n of replica u / n.  R = 3 x N = 100 gives 300 units: with wave_wgs = 1 one
workgroup's four waves take 75 units each and cross the replica boundaries mid-run."""
import ctypes as C

import numpy as np
import pytest

import common
import forces_ref as ref
from metropolismontecarlo_amd import structs
from test_gpu_deletion import edge_selection, make_batch, overlapping_molecules

pytestmark = pytest.mark.gpu

RCUT = 10.0
T = 298.15
MASS = np.array([15.9994, 1.00794, 1.00794])
EPS = 2.0 ** -52
ROWS = ("force", "torque", "vir", "atom", "ovl")


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def cfg4():
    return common.nist_arrays(4, "unwrapped")


@pytest.fixture(scope="module")
def diversified(cfg4):
    """NIST config 4, 3 replicas, each taken 300 device-proposed steps along its own chain."""
    b = make_batch(cfg4, 3)
    b.set_option("device_moves", 1)
    b.run(300, T, 0.3, 0.2, seed=4242)
    yield b
    b.close()


@pytest.fixture(scope="module")
def diversified_rows(diversified):
    """One full call with every row, shared (and left unchanged) by the tests that read it."""
    return diversified.forces(mass=MASS, details=True)


@pytest.fixture(scope="module")
def refs0(orc, cfg4, diversified):
    """forces_ref.molecule of every molecule of replica 0, computed once."""
    su = ref.setup(cfg4, orc, cfg4["box"], RCUT, RCUT)
    com, coords, S = diversified.get_replica(0)
    return [ref.molecule(su, com, coords, S, i, MASS) for i in range(diversified.n_mol)]


def subset(a, keep):
    keep = np.asarray(keep)
    n = keep.shape[0]
    at = (3 * keep[:, None] + np.arange(3)[None, :]).ravel()
    return dict(a, com=np.asarray(a["com"])[keep], coords=np.asarray(a["coords"]).reshape(-1, 3)[at],
                atype=np.asarray(a["atype"])[:3 * n], charge=np.asarray(a["charge"])[:3 * n])


# ---- every output against the restatement, on the three shapes ----------------------------------
def test_all_molecules_against_the_restatement(orc, cfg4, diversified, diversified_rows, refs0):
    """2250 units on the per-molecule image path (whole molecules, gate + 2 r_mol < L / 2), about 125
    neighbours inside the prefilter: two rounds of 64."""
    b, out = diversified, diversified_rows
    n = cfg4["com"].shape[0]
    assert out["force"].shape == (3, n, 3) and out["atom"].shape == (3, n, 3, 3) and out["ovl"].shape == (3, n)
    assert np.all(out["ovl"] == 0) and np.all(np.isfinite(out["atom"])) and np.all(out["vir"][..., 2] > 0)
    assert not np.array_equal(out["force"][0], out["force"][1])
    su = ref.setup(cfg4, orc, cfg4["box"], RCUT, RCUT)
    worst = ref.check(su, b, 0, np.arange(n), out, np.arange(n), MASS, what="img", refs=refs0)
    sel = edge_selection(n, 40, 1)
    for r in (1, 2):
        worst = max(worst, ref.check(su, b, r, sel, out, sel, MASS, what="img"))
    print("worst |x - ref| / A:", worst)
    # without masses t is 0 and nothing else changes
    bare = b.forces(details=True)
    assert np.all(bare["vir"][..., 2] == 0.0)
    for k in ("force", "torque", "atom", "ovl"):
        assert bare[k].tobytes() == out[k].tobytes(), k
    assert bare["vir"][..., :2].tobytes() == out["vir"][..., :2].tobytes()


def test_broken_molecules_take_the_per_pair_image(orc):
    """nist_arrays(4, "reference"): molecules stored broken across the box, r_mol is unbounded and
    the per-pair minimum image (vector1D) runs instead of the per-molecule one."""
    a = common.nist_arrays(4, "reference")
    n = a["com"].shape[0]
    sel = edge_selection(n, 40, 1)
    su = ref.setup(a, orc, a["box"], RCUT, RCUT)
    with make_batch(a, 2) as b:
        b.set_option("device_moves", 1)
        b.run(300, T, 0.3, 0.2, seed=77)
        out = b.forces(sel=sel, mass=MASS, details=True)
        assert np.all(out["ovl"] == 0) and out["atom"].shape == (2, 40, 3, 3)
        for r in range(2):
            print("worst", ref.check(su, b, r, sel, out, np.arange(40), MASS, what="per pair"))


def test_small_box_one_workgroup_crossing_replicas(orc):
    """Config 1 (100 molecules, nearly all inside the gate), R = 3 and wave_wgs = 1: four waves take
    75 units each and cross the replica boundaries."""
    a = common.nist_arrays(1, "unwrapped")
    n = a["com"].shape[0]
    su = ref.setup(a, orc, a["box"], RCUT, RCUT)
    with make_batch(a, 3) as b:
        b.set_option("device_moves", 1)
        b.run(120, T, 0.3, 0.2, seed=17)
        b.set_option("wave_wgs", 1)
        out = b.forces(mass=MASS, details=True)
        b.set_option("wave_wgs", 0)
        assert np.all(out["ovl"] == 0)
        for r in range(3):
            print("worst", ref.check(su, b, r, np.arange(n), out, np.arange(n), MASS, what="config 1"))


# ---- the reciprocal force alone -----------------------------------------------------------------
def test_reciprocal_force_alone(orc, cfg4):
    """Molecules 0, 64 and N - 1 of config 4 and others, all further apart than the cutoff (8 A here:
    0 and 64 are 8.4 A apart): no pair passes a gate, so the forces are the reciprocal part alone --
    restated on the batch's own 337-entry S(k) with orc.Ewald's kxyz and cfac."""
    L, rc = float(cfg4["box"]), 8.0
    com = np.asarray(cfg4["com"], dtype=float)
    n = com.shape[0]
    keep = [0, 64, n - 1]
    for j in range(n):
        d = ref.vector1D(com[j][None, :], com[keep], L)
        if j not in keep and np.all((d * d).sum(1) > (rc + 0.5) ** 2):
            keep.append(j)
    keep = sorted(keep)
    assert len(keep) >= 10
    a = subset(cfg4, keep)
    ew = orc.Ewald(5.6 / L, 5, 27, L, factor=structs.factor)
    q3 = np.asarray(cfg4["charge"][:3], dtype=float)
    with make_batch(a, 1, rcut=rc) as b:
        out = b.forces(details=True)
        _, coords, S = b.get_replica(0)
    assert S.shape[0] == ew.NKVECS == 337 and np.all(out["ovl"] == 0)
    assert np.all(out["vir"] == 0.0)                              # no pair: both virials are exact zeros
    for i in (0, 64, n - 1):
        k = keep.index(i)
        x = coords[3 * k:3 * k + 3]
        e = np.exp(2j * np.pi * (ew.kxyz @ x.T) / L)              # [k, a]
        terms = (ew.cfac[:, None, None] * ew.kxyz[:, None, :]) * (np.conj(S)[:, None] * e).imag[:, :, None]
        pre = (ew.factor * 4 * np.pi / L) * q3
        want = pre[:, None] * terms.sum(0)
        A = np.abs(pre)[:, None] * (np.abs(ew.cfac[:, None, None] * ew.kxyz[:, None, :])
                                    * (np.abs(S.real[:, None] * e.imag) + np.abs(S.imag[:, None] * e.real))[:, :, None]).sum(0)
        assert ref.close(out["atom"][0, k], want, A), (i, out["atom"][0, k], want)
        assert np.abs(want).max() > 1.0


# ---- fsum, launch shape, selection --------------------------------------------------------------
def test_fsum_bit_for_bit_and_launch_independence(diversified, diversified_rows):
    b, full = diversified, diversified_rows
    n = b.n_mol
    fsum, nfl = ref.host_sums(full["force"], full["torque"], full["vir"], full["ovl"])
    assert full["fsum"].tobytes() == fsum.tobytes() and np.all(full["fsum"][:, 0] == n)
    assert np.all(full["n_flagged"] == 0)
    n0 = np.array([4, 0, 9], dtype=np.int64)
    for wgs in (1, 2, 0):
        b.set_option("wave_wgs", wgs)
        res = b.forces(mass=MASS, details=True, n_flagged=n0.copy())
        for k in ROWS + ("fsum",):
            assert res[k].tobytes() == full[k].tobytes(), (wgs, k)
        assert np.array_equal(res["n_flagged"], n0)
    b.set_option("wave_wgs", 0)
    # fsum alone (no rows asked for) is the same
    assert b.forces(mass=MASS)["fsum"].tobytes() == full["fsum"].tobytes()
    # a selection with a duplicate: the same rows as the full call's, its own sums
    sel = np.array([700, 3, 64, 3, 749])
    res = b.forces(sel=sel, mass=MASS, details=True)
    assert res["atom"].shape == (b.R, 5, 3, 3)
    for k in ROWS:
        assert res[k].tobytes() == np.ascontiguousarray(full[k][:, sel]).tobytes(), k
    fsum, _ = ref.host_sums(res["force"], res["torque"], res["vir"], res["ovl"])
    assert res["fsum"].tobytes() == fsum.tobytes() and np.all(res["fsum"][:, 0] == 5)
    one = b.forces(sel=np.array([64], dtype=np.int64), mass=MASS, details=True)
    assert one["force"].tobytes() == np.ascontiguousarray(full["force"][:, [64]]).tobytes()


def test_sum_rules(diversified, diversified_rows, refs0):
    """sum F vanishes against sum_i A_i (replica 0, whose A_i the restatement has); sum w_lj against
    potential_ewald()'s virial with the header's factor, 2 (virial - coulomb / 3) (checked on the
    oracle in tests/test_forces_host.py)."""
    b, out = diversified, diversified_rows
    tot = b.potential_ewald(as_array=True)
    for r in range(b.R):
        want = 2 * (tot["virial"][r] - tot["coulomb"][r] / 3.0)
        print(r, out["fsum"][r, 7], want)
        assert common.rel(out["fsum"][r, 7], want) < 1e-12
    A = sum(m["A_force"] for m in refs0)
    print("sum F", out["fsum"][:, 4:7], "sum A", A)
    assert np.all(np.abs(out["fsum"][0, 4:7]) <= 1e-12 * A)


# ---- consistency with mmc_batch_deletion --------------------------------------------------------
def test_rigid_displacement_against_deletion(orc, cfg4):
    """Molecule i moved rigidly by +-h (COM too): U(N without i) does not change, so the central
    difference of deletion's dU_i is -F_i.  Only molecules with no neighbour within 4 h of the gate
    are taken (forces_ref lists them).  Tolerance: the finite difference's own error -- h against
    h / 2, plus eps |dU| / h -- times 10."""
    a, h = cfg4, 1.0e-3
    L = float(a["box"])
    com0, x0 = np.asarray(a["com"], dtype=float), np.asarray(a["coords"], dtype=float).reshape(-1, 3)
    su = ref.setup(a, orc, L, RCUT, RCUT)
    n = com0.shape[0]
    with make_batch(a, 1) as b:
        _, _, S = b.get_replica(0)
        F = b.forces(details=True)["force"][0]
        picked = []
        for i in (0, 63, 64, 127, 128, n - 1, 300, 500):
            m = ref.molecule(su, com0, x0, S, i)
            if m["gate_margin"] > 4 * h and ref.fd_safe(m, 2 * h):
                picked.append(i)
            if len(picked) == 3:
                break
        assert len(picked) == 3

        def du(i, d, s):
            c, x = com0.copy(), x0.copy()
            c[i, d] += s
            x[3 * i:3 * i + 3, d] += s
            b.set_replica(0, c, x)
            b.recip_long()
            t = b.deletion(T, sel=np.array([i]), details=True)["du"][0, 0]
            return (t[0] + t[1]) + t[2], np.abs(t).sum()
        worst = 0.0
        for i in picked:
            for d in range(3):
                (up, mag), (dn, _) = du(i, d, h), du(i, d, -h)
                (up2, _), (dn2, _) = du(i, d, 0.5 * h), du(i, d, -0.5 * h)
                d1, d2 = (up - dn) / (2 * h), (up2 - dn2) / h
                allowed = 10 * (abs(d1 - d2) + EPS * mag / (0.5 * h))
                worst = max(worst, abs(-d2 - F[i, d]) / allowed)
                assert abs(-d2 - F[i, d]) <= allowed, (i, d, -d2, F[i, d], allowed)
        print("molecules", picked, "h", h, "worst ratio", worst)


# ---- flags --------------------------------------------------------------------------------------
def test_flags_overlap_and_singular_inertia(cfg4):
    """Replica 1: an H of molecule 10 placed 0.5 A from the O of molecule 300 (r^2 = 0.25 < 0.5,
    opposite charges): both get bit 0, zeros in their rows, are left out of fsum and counted.
    Replica 2: one molecule laid out along x through its stored COM -- I is singular: bit 1."""
    a = cfg4
    L, n = float(a["box"]), a["com"].shape[0]
    j, m = 10, 300
    com, coords = np.asarray(a["com"], dtype=float), np.asarray(a["coords"], dtype=float).reshape(-1, 3)
    placed = None
    for d in ((0.5, 0, 0), (-0.5, 0, 0), (0, 0.5, 0), (0, -0.5, 0), (0, 0, 0.5), (0, 0, -0.5)):
        shift = coords[3 * m] + np.array(d) - coords[3 * j + 1]
        c1, x1 = com.copy(), coords.copy()
        c1[j] += shift
        x1[3 * j:3 * j + 3] += shift
        wrap = np.floor(c1[j] / L) * L
        c1[j] -= wrap
        x1[3 * j:3 * j + 3] -= wrap
        if overlapping_molecules(x1, a["charge"], L) == {j, m}:
            placed = (c1, x1)
            break
    assert placed is not None
    line = None
    for k in (20, 21, 22, 23, 24, 25):
        x2 = coords.copy()
        x2[3 * k:3 * k + 3] = com[k] + np.array([[0.0, 0, 0], [1.0, 0, 0], [-1.0, 0, 0]])
        if not overlapping_molecules(x2, a["charge"], L):
            line = (k, x2)
            break
    assert line is not None
    k, x2 = line
    with make_batch(a, 3) as b:
        b.set_replica(1, *placed)
        b.set_replica(2, com, x2)
        b.recip_long()
        nf0 = np.array([5, 0, 1], dtype=np.int64)
        res = b.forces(mass=MASS, details=True, n_flagged=nf0.copy())
        bare = b.forces(details=True)                  # without masses nothing of replica 2 is singular
    ovl = res["ovl"]
    others = np.ones(n, dtype=bool)
    others[[j, m]] = False
    assert np.all(ovl[0] == 0) and np.all(ovl[1][[j, m]] == 1) and np.all(ovl[1][others] == 0)
    assert ovl[2, k] == 2 and np.count_nonzero(ovl[2]) == 1
    for name in ("force", "torque", "vir", "atom"):
        assert np.all(res[name][1][[j, m]] == 0.0) and np.all(res[name][2][k] == 0.0), name
        assert np.all(np.isfinite(res[name]))
    assert np.any(res["force"][1][others] != 0.0)
    assert np.array_equal(res["n_flagged"], nf0 + np.array([0, 2, 1]))
    assert np.array_equal(res["fsum"][:, 0], [n, n - 2, n - 1])
    fsum, _ = ref.host_sums(res["force"], res["torque"], res["vir"], ovl)
    assert res["fsum"].tobytes() == fsum.tobytes()
    assert np.all(bare["ovl"][2] == 0) and np.any(bare["force"][2, k] != 0.0) and bare["fsum"][2, 0] == n


# ---- read-only ----------------------------------------------------------------------------------
def test_the_call_is_read_only(cfg4):
    R = 2
    twins = [make_batch(cfg4, R), make_batch(cfg4, R)]
    chains = []
    for b in twins:
        b.set_option("device_moves", 1)
        chains.append(b.new_chains(b.potential_ewald(as_array=True)["energy"]))
    b = twins[0]
    before = [b.get_replica(r) for r in range(R)]
    pe = b.potential_ewald(as_array=True)
    b.forces(mass=MASS)
    for x, y in zip(before, [b.get_replica(r) for r in range(R)]):
        for u, v in zip(x, y):
            assert u.tobytes() == v.tobytes()
    assert pe.tobytes() == b.potential_ewald(as_array=True).tobytes()
    rng = np.random.default_rng(8)
    for blk in range(3):
        for b, c in zip(twins, chains):
            b.run_chains(c, 200, T, seed=808)
        twins[0].forces(sel=rng.integers(0, 750, size=16), mass=MASS, details=True)
    assert chains[0].tobytes() == chains[1].tobytes()
    for r in range(R):
        for u, v in zip(twins[0].get_replica(r), twins[1].get_replica(r)):
            assert u.tobytes() == v.tobytes()
    assert twins[0].potential_ewald(as_array=True).tobytes() == twins[1].potential_ewald(as_array=True).tobytes()
    for b in twins:
        b.close()


# ---- refusals -----------------------------------------------------------------------------------
def test_refusals_leave_outputs_untouched(cfg4):
    from metropolismontecarlo_amd import _lib
    a = cfg4
    R, n = 2, a["com"].shape[0]
    L = _lib.lib()

    def raw(b, n_sel=0, sel=None, mass=None, want=None):
        """The C entry point with every output given and filled with sentinels: its status, and that
        an error left all seven alone."""
        nn = max(n if sel is None else len(sel), 1)
        outs = [np.full((R, nn, 3), -1.5), np.full((R, nn, 3), -1.5), np.full((R, nn, 3), -1.5),
                np.full((R, nn, 9), -1.5), np.full((R, 9), 7.5)]
        nf, ovl = np.full(R, 3, dtype=np.int64), np.full((R, nn), 9, dtype=np.uint8)
        sel_a = None if sel is None else np.ascontiguousarray(sel, dtype=np.int32)
        mass_a = None if mass is None else np.ascontiguousarray(mass, dtype=np.float64)
        st = L.mmc_batch_forces(
            b._h, n_sel, None if sel_a is None else sel_a.ctypes.data_as(C.POINTER(C.c_int32)),
            None if mass_a is None else mass_a.ctypes.data_as(_lib._dp),
            *[x.ctypes.data_as(_lib._dp) for x in outs], nf.ctypes.data_as(_lib._i64p),
            ovl.ctypes.data_as(C.POINTER(C.c_uint8)))
        untouched = (all(np.all(x == -1.5) for x in outs[:4]) and np.all(outs[4] == 7.5) and np.all(nf == 3)
                     and np.all(ovl == 9))
        if want is not None:
            assert st == want, (st, want, L.mmc_last_error())
            assert untouched == (want != _lib.MMC_OK)
        return st

    # per-replica boxes
    with make_batch(a, R) as b:
        b.set_boxes([a["box"], a["box"] * 1.01], 5.6)
        raw(b, want=_lib.MMC_ERR_UNSUPPORTED)
    # a cutoff the erfc table does not cover (r_cut^2 + 100 > 256): no table kernels
    with make_batch(a, R, rcut=14.0) as b:
        raw(b, want=_lib.MMC_ERR_UNSUPPORTED)
    with make_batch(a, R) as b:
        # Wolf style, then back to Ewald with S(k) stale
        b.set_coulomb_style("wolf")
        raw(b, want=_lib.MMC_ERR_UNSUPPORTED)
        b.set_coulomb_style("ewald")
        raw(b, want=_lib.MMC_ERR_STATE)
        assert b"mmc_batch_recip_long" in L.mmc_last_error()
        b.recip_long()
        raw(b, mass=MASS, want=_lib.MMC_OK)
        # proposals outstanding
        com, coords = np.asarray(a["com"]), np.asarray(a["coords"])
        b.eval(np.full(R, 3), np.tile(com[2], (R, 1)), np.tile(coords[6:9], (R, 1, 1)))
        raw(b, want=_lib.MMC_ERR_STATE)
        b.settle(np.zeros(R, dtype=np.int32))
        # bad arguments
        raw(b, n_sel=0, sel=[], want=_lib.MMC_ERR_ARG)
        raw(b, n_sel=3, sel=[0, n, 5], want=_lib.MMC_ERR_ARG)
        raw(b, n_sel=3, sel=[0, -1, 5], want=_lib.MMC_ERR_ARG)
        for mass in ((0.0, 1.0, 1.0), (16.0, -1.0, 1.0), (16.0, 1.0, float("nan")), (float("inf"), 1.0, 1.0)):
            raw(b, mass=mass, want=_lib.MMC_ERR_ARG)
        assert L.mmc_batch_forces(b._h, 0, None, None, None, None, None, None, None, None, None) == _lib.MMC_ERR_ARG
        # the wrapper raises the library's status
        nf = np.full(R, 3, dtype=np.int64)
        with pytest.raises(_lib.MMCError) as ei:
            b.forces(mass=(16.0, 0.0, 1.0), n_flagged=nf)
        assert ei.value.status == _lib.MMC_ERR_ARG and np.all(nf == 3)
        # ... and after all that the call works
        raw(b, n_sel=2, sel=[5, n - 1], want=_lib.MMC_OK)
        res = b.forces()
        assert np.all(res["fsum"][:, 0] == n) and np.all(res["fsum"][:, 1] > 0)
