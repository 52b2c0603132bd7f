"""Deletion energies (mmc_batch_deletion) against the oracle, against mmc_batch_widom_at and against
the rules the header states.

The reference has no deletion code; dU_i is defined through its total energy (include/mmc_hip.h):
what potential(..., "ewald") loses when molecule i is taken out.  The oracle is asked exactly that,
term by term (deletion_ref.oracle_terms):
  d_lj    == orc.lj_poly_du(i)
  d_real  == orc.ewald_short(i)                      (0 when it reports an overlap)
  d_recip == factor (recip_long(N) - recip_long(N \\ i)) + orc.ewald_self(molecule i's charges)
Tolerance per term: 1e-9 K absolute plus 1e-13 of the term (common.widom_close: the erfc table's
error, tests/test_gpu_table.py).  Histograms are compared by integer equality, the per-replica sums
bit for bit with the fixed-order host sums of deletion_ref (exp may differ by an ulp: 1e-14).

Launch shape: k_deletion_wave runs WV_WAVES = 4 waves per workgroup on at most "wave_wgs" workgroups;
unit u is entry u % n of replica u / n.  R = 3 x N = 100 gives 300 units: with wave_wgs = 1 one
workgroup's four waves take 75 units each and cross the replica boundaries mid-run."""
import numpy as np
import pytest

import common
import deletion_ref as ref
from metropolismontecarlo_amd import observables as obs
from metropolismontecarlo_amd import structs

pytestmark = pytest.mark.gpu

RCUT = 10.0
T = 298.15
# dU carries the self term of the molecule (about -19 000 K at kappa = 5.6 / 30 A, -28 000 K at
# 5.6 / 20 A) without the intramolecular term that cancels most of it (include/mmc_hip.h)
BINS = (120, -60000.0, 0.0)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def make_batch(a, R, rcut=RCUT, recip=True):
    from metropolismontecarlo_amd.device import Batch
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
              5.6 / a["box"], structs.factor, rcut, rcut)
    if recip:
        b.recip_long()
    return b


def edge_selection(n, count, seed):
    """`count` molecules: the lane and block edges of the scan (0, 63, 64, 127, 128, N - 1) and
    random others."""
    must = [0, 63, 64, 127, 128, n - 1]
    rng = np.random.default_rng(seed)
    rest = [int(i) for i in rng.permutation(n) if i not in must][:count - len(must)]
    return np.array(sorted(must + rest))


def total_du(du):
    return (du[..., 0] + du[..., 1]) + du[..., 2]


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


# ---- 1, 2: oracle parity on both image paths ----------------------------------------------------
def test_all_molecules_against_the_oracle(orc, cfg4, diversified):
    """2250 units on the per-molecule image path (whole molecules, gate + 2 r_mol < L / 2)."""
    b = diversified
    n = cfg4["com"].shape[0]
    res = b.deletion(T, details=True)
    du, ovl = res["du"], res["ovl"]
    assert du.shape == (3, n, 3) and ovl.shape == (3, n)
    assert np.all(ovl == 0) and np.all(np.isfinite(du))
    assert not np.array_equal(du[0], du[1])
    sel = edge_selection(n, 40, 1)
    for r in range(b.R):
        ref.check(orc, cfg4, b, r, sel, du[r][sel], ovl[r][sel], RCUT, RCUT, what="img")
    # the reciprocal term restated in numpy on the batch's own S(k) (the reference's 337 entries)
    L = float(cfg4["box"])
    ew = orc.Ewald(5.6 / L, 5, 27, L, factor=structs.factor)
    q3 = np.asarray(cfg4["charge"][:3], dtype=float)
    _, coords, S = b.get_replica(2)
    for i in (0, 64, n - 1):
        x = coords[3 * i:3 * i + 3]
        s = (q3[None, :] * np.exp(2j * np.pi * (ew.kxyz @ x.T) / L)).sum(1)
        want = ew.factor * (ew.cfac * (2 * (np.conj(S) * s).real - (s * np.conj(s)).real)).sum() \
            + orc.ewald_self(ew, q3)
        assert abs(du[2, i, 2] - want) <= 1e-12 * abs(want), (i, du[2, i, 2], want)


def test_broken_molecules_take_the_per_pair_image(orc):
    """nist_arrays(4, "reference"): molecules stored broken across the box, r_mol is unbounded and
    the per-pair minimum image (vector1D) runs instead of the per-molecule one."""
    a = common.nist_arrays(4, "reference")
    n = a["com"].shape[0]
    sel = edge_selection(n, 40, 1)
    with make_batch(a, 2) as b:
        b.set_option("device_moves", 1)
        b.run(300, T, 0.3, 0.2, seed=77)
        res = b.deletion(T, details=True)
        assert np.all(res["ovl"] == 0)
        for r in range(2):
            ref.check(orc, a, b, r, sel, res["du"][r][sel], res["ovl"][r][sel], RCUT, RCUT, what="per pair")


# ---- 3: against existing code -------------------------------------------------------------------
def test_deletion_is_the_insertion_into_the_others(cfg4):
    """Molecule i's terms equal what mmc_batch_widom_at returns for i's coordinates in a batch of
    the other N - 1 molecules."""
    a = cfg4
    n = a["com"].shape[0]
    with make_batch(a, 1) as b:
        res = b.deletion(T, details=True)
    bad = []
    for i in (0, 63, 64, 400, 512, n - 1):
        com, coords = ref.without(a, a["com"], a["coords"], i)
        rest = dict(a, com=com, coords=coords, atype=np.asarray(a["atype"])[:3 * (n - 1)],
                    charge=np.asarray(a["charge"])[:3 * (n - 1)])
        with make_batch(rest, 1) as bw:
            _, no, du, ovl = bw.widom_at(ref.record(a["com"], a["coords"], i)[None, None], T)
        assert ovl[0, 0] == 0 and no[0] == 0
        for k, name in enumerate(("lj", "real", "recip")):
            if not common.widom_close(res["du"][0, i, k], du[0, 0, k]):
                bad.append((i, name, res["du"][0, i, k], du[0, 0, k]))
    assert not bad, bad


# ---- 4: sum rules -------------------------------------------------------------------------------
def test_sum_rules(cfg4, diversified):
    """esum against mmc_batch_potential_ewald's totals: twice the pair totals (the relation is
    checked on the oracle in tests/test_deletion_host.py)."""
    b = diversified
    n = cfg4["com"].shape[0]
    tot = b.potential_ewald(as_array=True)
    res = b.deletion(T)
    for r in range(b.R):
        print(r, res["esum"][r], 2 * tot["lj"][r], 2 * tot["real"][r])
        assert common.rel(res["esum"][r, 0], 2 * tot["lj"][r]) < 1e-12
        assert common.rel(res["esum"][r, 1], 2 * tot["real"][r]) < 1e-12
        assert res["esum"][r, 3] == n
    assert np.all(res["n_flagged"] == 0)


# ---- 5: launch shape and reproducibility --------------------------------------------------------
def test_launch_shape_and_reproducibility():
    a = common.nist_arrays(1, "unwrapped")
    R, n = 3, a["com"].shape[0]
    rng = np.random.default_rng(3)
    b0 = rng.random(R) * 1e-50                  # (the weights are exp(-100) and less: see BINS)
    n0 = rng.integers(0, 5, size=R).astype(np.int64)
    runs = []
    with make_batch(a, R, rcut=9.0) as b:
        b.set_option("device_moves", 1)
        b.run(120, T, 0.3, 0.2, seed=17)
        for wgs in (0, 1, 2, 0):
            b.set_option("wave_wgs", wgs)
            tot = b.deletion(T, bins=BINS, boltz_sum=b0.copy(), n_flagged=n0.copy(), details=True)
            per = b.deletion(T, bins=BINS, per_replica=True, boltz_sum=b0.copy(), n_flagged=n0.copy())
            runs.append((tot, per))
        b.set_option("wave_wgs", 0)
    tot, per = runs[0]
    for other_tot, other_per in runs[1:]:
        for x, y in ((tot, other_tot), (per, other_per)):
            assert sorted(x) == sorted(y)
            for k in x:
                assert x[k].tobytes() == y[k].tobytes(), k
    du, ovl = tot["du"], tot["ovl"]
    assert du.shape == (R, n, 3) and not np.array_equal(du[0], du[1])
    esum, boltz, nfl = ref.host_sums(du, ovl, T, b0, n0)
    assert tot["esum"].tobytes() == esum.tobytes() == per["esum"].tobytes()
    assert np.all(np.abs(tot["boltz_sum"] - boltz) <= 1e-14 * np.abs(boltz)), (tot["boltz_sum"], boltz)
    assert tot["boltz_sum"].tobytes() == per["boltz_sum"].tobytes() and np.all(tot["boltz_sum"] > b0)
    assert np.array_equal(tot["n_flagged"], nfl) and np.array_equal(per["n_flagged"], nfl)
    d = total_du(du)
    rows = np.stack([ref.energy_bins(d[r][ovl[r] == 0], *BINS) for r in range(R)])
    assert per["hist"].dtype == np.uint64 and per["hist"].shape == (R, BINS[0] + 2)
    assert np.array_equal(per["hist"], rows)
    assert np.array_equal(tot["hist"], rows.sum(0)) and np.array_equal(per["hist"].sum(0), tot["hist"])
    assert np.array_equal(tot["hist"], obs.energy_bins(d[ovl == 0], *BINS))
    assert tot["hist"][1:-1].sum() > 0.9 * R * n          # the grid holds the distribution
    # a grid between the quartiles of the same values: both outer slots fill
    lo, hi = (float(x) for x in np.quantile(d, (0.25, 0.75)))
    with make_batch(a, R, rcut=9.0) as b:
        b.set_option("device_moves", 1)
        b.run(120, T, 0.3, 0.2, seed=17)
        res = b.deletion(T, bins=(7, lo, hi), details=True)
        assert res["du"].tobytes() == du.tobytes()
        assert np.array_equal(res["hist"], ref.energy_bins(d[ovl == 0], 7, lo, hi))
        assert res["hist"][0] > 0 and res["hist"][-1] > 0 and res["hist"].sum() == R * n


# ---- 6: selection -------------------------------------------------------------------------------
def test_selection_with_a_duplicate(diversified):
    b = diversified
    full = b.deletion(T, bins=BINS, per_replica=True, details=True)
    sel = np.array([700, 3, 64, 3, 749])
    res = b.deletion(T, sel=sel, bins=BINS, per_replica=True, details=True)
    assert res["du"].shape == (b.R, 5, 3)
    assert res["du"].tobytes() == np.ascontiguousarray(full["du"][:, sel]).tobytes()
    assert res["ovl"].tobytes() == np.ascontiguousarray(full["ovl"][:, sel]).tobytes()
    assert np.all(res["esum"][:, 3] == 5)
    esum, boltz, nfl = ref.host_sums(res["du"], res["ovl"], T)
    assert res["esum"].tobytes() == esum.tobytes()
    assert np.all(np.abs(res["boltz_sum"] - boltz) <= 1e-14 * np.abs(boltz))
    d = total_du(res["du"])
    assert np.array_equal(res["hist"], np.stack([ref.energy_bins(d[r], *BINS) for r in range(b.R)]))
    # other integer types and a single molecule
    one = b.deletion(T, sel=np.array([64], dtype=np.int64), details=True)
    assert one["du"].tobytes() == np.ascontiguousarray(full["du"][:, [64]]).tobytes()


# ---- 7: a constructed overlap -------------------------------------------------------------------
def overlapping_molecules(coords, charge, box):
    """Molecules with an atom closer than r^2 = 0.5 to an atom of opposite charge of another
    molecule (minimum image per pair), by brute force."""
    x = np.asarray(coords, dtype=float)
    q = np.asarray(charge, dtype=float)[:x.shape[0]]
    out = set()
    for i in range(x.shape[0]):
        d = x - x[i]
        d -= box * np.round(d / box)
        hit = np.nonzero(((d * d).sum(1) < 0.5) & (q * q[i] < 0) & (np.arange(x.shape[0]) // 3 != i // 3))[0]
        if hit.size:
            out.add(i // 3)
            out.update(int(h) // 3 for h in hit)
    return out


def test_constructed_overlap_and_coincident_atoms(cfg4):
    """Replica 1: an H of molecule 10 placed 0.5 A from the O of molecule 300 (r^2 = 0.25 < 0.5,
    opposite charges: the overlap of ewalds.jl:359).  Replica 2: molecule 10 placed exactly on
    molecule 300 (LJ gives Inf - Inf: a non-finite dU, no overlap).  Replica 0 is left alone."""
    a = cfg4
    L, n = float(a["box"]), a["com"].shape[0]
    j, m = 10, 300
    com, coords = np.asarray(a["com"], dtype=float), np.asarray(a["coords"], dtype=float)
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
    c2, x2 = com.copy(), coords.copy()
    c2[j] = com[m]
    x2[3 * j:3 * j + 3] = coords[3 * m:3 * m + 3]
    with make_batch(a, 3) as b:
        before = b.deletion(T, bins=BINS, per_replica=True, details=True)
        assert np.all(before["ovl"] == 0)
        b.set_replica(1, *placed)
        b.set_replica(2, c2, x2)
        b.recip_long()
        nf0 = np.array([5, 0, 1], dtype=np.int64)
        res = b.deletion(T, bins=BINS, per_replica=True, n_flagged=nf0.copy(), details=True)
    du, ovl = res["du"], res["ovl"]
    others = np.ones(n, dtype=bool)
    others[[j, m]] = False
    assert np.all(ovl[1][[j, m]] == 1) and np.all(du[1][[j, m], 1] == 0.0) and np.all(ovl[1][others] == 0)
    assert np.all(ovl[2][[j, m]] == 2) and not np.any(np.isfinite(total_du(du[2][[j, m]])))
    assert np.all(ovl[2][others] == 0)
    assert np.array_equal(res["n_flagged"], nf0 + np.array([0, 2, 2]))
    assert np.array_equal(res["esum"][:, 3], [n, n - 2, n - 2])
    assert np.array_equal(res["hist"].sum(1), [n, n - 2, n - 2])
    esum, boltz, _ = ref.host_sums(du, ovl, T)
    assert res["esum"].tobytes() == esum.tobytes() and np.all(np.isfinite(res["boltz_sum"]))
    assert np.all(np.abs(res["boltz_sum"] - boltz) <= 1e-14 * np.abs(boltz))
    d = total_du(du)
    for r in range(3):
        assert np.array_equal(res["hist"][r], ref.energy_bins(d[r][ovl[r] == 0], *BINS)), r
    # replica 0 is what it was
    assert du[0].tobytes() == before["du"][0].tobytes() and np.array_equal(res["hist"][0], before["hist"][0])
    assert res["esum"][0].tobytes() == before["esum"][0].tobytes()


# ---- 10: read-only ------------------------------------------------------------------------------
def test_the_call_is_read_only(cfg4):
    R = 4
    twins = [make_batch(cfg4, R), make_batch(cfg4, R)]
    chains = []
    for b in twins:
        b.set_option("device_moves", 1)
        e = b.potential_ewald(as_array=True)["energy"]
        chains.append(b.new_chains(e))
    b = twins[0]
    before = [b.get_replica(r) for r in range(R)]
    pe = b.potential_ewald(as_array=True)
    b.deletion(T, bins=BINS)
    after = [b.get_replica(r) for r in range(R)]
    for x, y in zip(before, after):
        for u, v in zip(x, y):
            assert u.tobytes() == v.tobytes()
    assert pe.tobytes() == b.potential_ewald(as_array=True).tobytes()
    acc = np.zeros(R)
    rng = np.random.default_rng(8)
    for blk in range(4):
        for b, c in zip(twins, chains):
            b.run_chains(c, 200, T, seed=808)
        twins[0].deletion(T, sel=rng.integers(0, 750, size=16), bins=BINS, boltz_sum=acc)
    assert chains[0].tobytes() == chains[1].tobytes()
    for r in range(R):
        for u, v in zip(twins[0].get_replica(r), twins[1].get_replica(r)):
            assert u.tobytes() == v.tobytes()
    assert np.all(acc > 0)
    for b in twins:
        b.close()


# ---- 12: refusals -------------------------------------------------------------------------------
def test_refusals_leave_outputs_untouched(cfg4):
    from metropolismontecarlo_amd import _lib
    a = cfg4
    R, n = 2, a["com"].shape[0]
    L = _lib.lib()
    import ctypes as C

    def raw(b, n_sel=0, sel=None, temp=T, bins=BINS, per_replica=0, want=None):
        """The C entry point with every output given and filled with sentinels: its status, and that
        an error left all six alone."""
        nn = n if sel is None else len(sel)
        hist = np.full((R, bins[0] + 2) if per_replica else (bins[0] + 2,), 77, dtype=np.uint64)
        esum, bs, nf = np.full((R, 4), 7.5), np.full(R, 2.5), np.full(R, 3, dtype=np.int64)
        du, ovl = np.full((R, max(nn, 1), 3), -1.5), np.full((R, max(nn, 1)), 9, dtype=np.uint8)
        sel_a = None if sel is None else np.ascontiguousarray(sel, dtype=np.int32)
        st = L.mmc_batch_deletion(
            b._h, n_sel, None if sel_a is None else sel_a.ctypes.data_as(C.POINTER(C.c_int32)), temp,
            bins[0], bins[1], bins[2], per_replica, hist.ctypes.data_as(C.POINTER(C.c_uint64)),
            esum.ctypes.data_as(_lib._dp), bs.ctypes.data_as(_lib._dp), nf.ctypes.data_as(_lib._i64p),
            du.ctypes.data_as(_lib._dp), ovl.ctypes.data_as(C.POINTER(C.c_uint8)))
        untouched = (np.all(hist == 77) and np.all(esum == 7.5) and np.all(bs == 2.5) and np.all(nf == 3)
                     and np.all(du == -1.5) and np.all(ovl == 9))
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
        raw(b, want=_lib.MMC_OK)
        # proposals outstanding
        com, coords = np.asarray(a["com"]), np.asarray(a["coords"])
        b.eval(np.full(R, 3), np.tile(com[2], (R, 1)), np.tile(coords[6:9], (R, 1, 1)))
        raw(b, want=_lib.MMC_ERR_STATE)
        b.settle(np.zeros(R, dtype=np.int32))
        # (a volume trial in flight needs a batch of one replica: tests/test_gpu_deletion_paths.py)
        # bad arguments
        for temp in (0.0, -5.0, float("nan"), float("inf")):
            raw(b, temp=temp, want=_lib.MMC_ERR_ARG)
        for bins in ((0, -1.0, 1.0), (4097, -1.0, 1.0), (10, 1.0, 1.0), (10, 2.0, 1.0),
                     (10, float("nan"), 1.0), (10, 0.0, float("inf"))):
            raw(b, bins=bins, want=_lib.MMC_ERR_ARG)
        raw(b, n_sel=0, sel=[], want=_lib.MMC_ERR_ARG)
        raw(b, n_sel=3, sel=[0, n, 5], want=_lib.MMC_ERR_ARG)
        raw(b, n_sel=3, sel=[0, -1, 5], want=_lib.MMC_ERR_ARG)
        assert L.mmc_batch_deletion(b._h, 0, None, T, 10, -1.0, 1.0, 0, None, None, None, None, None,
                                    None) == _lib.MMC_ERR_ARG
        # the wrapper raises the library's status
        bs = np.full(R, 2.5)
        with pytest.raises(_lib.MMCError) as ei:
            b.deletion(-1.0, boltz_sum=bs)
        assert ei.value.status == _lib.MMC_ERR_ARG and np.all(bs == 2.5)
        # ... and after all that the call works; a histogram is not needed, nor its grid looked at
        raw(b, n_sel=2, sel=[5, n - 1], per_replica=1, want=_lib.MMC_OK)
        res = b.deletion(T)
        assert "hist" not in res and np.all(res["esum"][:, 3] == n) and np.all(res["boltz_sum"] > 0)
