"""mmc_batch_rdf_sites and mmc_batch_dipoles against their numpy restatement
(tests/structure_ref.py: the pair loop of Ewald/gr.jl:60-91 for the six slot pairs; vector1D
dipoles).  Every histogram comparison is exact integer equality.

Launch shape: k_rdf_sites_wave's unit is a 64 x 64 tile of the i < j triangle, K (K + 1) / 2 per
replica with K = ceil(N / 64); wave W of the launch's NW takes the contiguous run
[n_tiles W / NW, n_tiles (W + 1) / NW).  The launch has at most "wave_wgs" workgroups of four
waves (default four per compute unit).  With wave_wgs = 1 four waves share everything, so each
takes many tiles and crosses replica boundaries; for the default grid to give a wave several tiles
R must exceed 3 x 16 waves x n_cus / tiles per replica (the reasoning the headline-shape tests use
for k_move_eval_wave: units per persistent wave = units / resident waves)."""
import numpy as np
import pytest

import common
import structure_ref as ref
from metropolismontecarlo_amd import _lib, structs

pytestmark = pytest.mark.gpu

RCUT = 10.0
T, DR, DPHI = 298.15, 0.3, 0.2
ALPHA = 5.6


def make_batch(a, R, rcut=RCUT):
    from metropolismontecarlo_amd.device import Batch
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
              ALPHA / a["box"], structs.factor, rcut, rcut)
    b.recip_long()
    return b


def want_rows(b, boxes, numbins, r_max=0.0):
    """[R, 6, numbins + 1] from the batch's own coordinates, each replica at its box."""
    return np.stack([ref.six_rows(b.get_replica(r)[1], float(boxes[r]), numbins, r_max)
                     for r in range(b.R)])


def check_batch(b, boxes, numbins, r_max=0.0, what="", want=None):
    if want is None:
        want = want_rows(b, boxes, numbins, r_max)
    per = b.rdf_sites(numbins, r_max, per_replica=True)
    tot = b.rdf_sites(numbins, r_max)
    assert per.dtype == np.uint64 and per.shape == (b.R, 6, numbins + 1) and tot.shape == (6, numbins + 1)
    for r in range(b.R):
        for k in range(6):
            assert np.array_equal(per[r, k], want[r, k]), (what, "replica", r, "row", k)
    assert np.array_equal(tot, want.sum(0)), what
    assert np.array_equal(per.sum(0), tot), what
    return per, tot


def small_system(n_mol, box, seed):
    return common.random_system(n_mol, box, seed=seed, na_choices=(3,))


@pytest.mark.parametrize("variant", ["unwrapped", "reference"])
def test_six_rows_match_the_restatement_on_nist_config_1(variant):
    a = common.nist_arrays(1, variant)
    box, numbins = a["box"], 100
    with make_batch(a, 3) as b:
        b.run(150, 298.15, 0.4, 0.2, seed=2, n_groups=1)          # replicas diverge
        per, tot = check_batch(b, [box] * 3, numbins, what=variant)
        assert not np.array_equal(per[0], per[1])
        assert tot.sum() > 0 and tot[0, :10].sum() == 0            # no O-O closer than 1 A
        # the one-site call on each slot, r_max = 0: gr.jl's own bin width
        for site, row in ((0, 0), (1, 3), (2, 5)):
            assert np.array_equal(tot[row], b.rdf(site, numbins)), site
        # cross rows hold every ordered molecule pair at most once
        n = a["com"].shape[0]
        assert tot[1].sum() <= 3 * n * (n - 1) and tot[0].sum() <= 3 * n * (n - 1) // 2


def test_other_ranges_and_bin_counts():
    a = common.nist_arrays(1, "unwrapped")
    box = a["box"]
    with make_batch(a, 2) as b:
        b.run(100, T, DR, DPHI, seed=5, n_groups=1)
        check_batch(b, [box] * 2, 64, r_max=RCUT, what="cutoff")
        check_batch(b, [box] * 2, 1, what="one bin")
        check_batch(b, [box] * 2, 1, r_max=3.3, what="one bin, r_max")
        check_batch(b, [box] * 2, 77, r_max=0.37 * box, what="77 bins")
        check_batch(b, [box] * 2, 700, what="two waves per workgroup")     # 104 (700 + 2) > 64 KB
        check_batch(b, [box] * 2, 1300, r_max=box / 2, what="one wave per workgroup")


def test_750_molecules():
    a = common.nist_arrays(4, "unwrapped")
    with make_batch(a, 2) as b:
        b.set_option("device_moves", 1)
        b.run(300, T, DR, DPHI, seed=4242)
        per, tot = check_batch(b, [a["box"]] * 2, 200, what="cfg4")
        assert np.array_equal(tot[0], b.rdf(0, 200))
        check_batch(b, [a["box"]] * 2, 50, r_max=RCUT, what="cfg4, cutoff")


@pytest.mark.parametrize("n_mol", [2, 3, 65, 129])
def test_tiny_and_odd_systems(n_mol):
    """One tile, a diagonal tile with one chosen molecule in its last block (65 = 64 + 1), three
    blocks with a one-molecule last block (129)."""
    box = 22.0 if n_mol > 3 else 21.0
    a = small_system(n_mol, box, seed=100 + n_mol)
    with make_batch(a, 3) as b:
        check_batch(b, [box] * 3, 40, what=f"n_mol {n_mol}")
        check_batch(b, [box] * 3, 25, r_max=RCUT, what=f"n_mol {n_mol}, cutoff")
        d = b.dipoles()
        mu = ref.molecule_dipoles(*b.get_replica(0)[:2], a["charge"], box)
        assert np.all(np.abs(d[0] - mu.sum(0)) <= 1e-12 * np.abs(mu).sum(0) + 1e-300)


@pytest.mark.parametrize("numbins", [628, 629, 1168, 1169, 2046])
def test_the_bin_counts_at_which_a_workgroup_loses_waves(numbins):
    """The thresholds and a wave's six 32-bit rows, 8 rs + nw 24 rs bytes with rs = numbins + 2, within
    65536: four waves up to 628 bins, two from 629 to 1168, one from 1169 to the 2046 allowed.  Three
    blocks a replica, and with wave_wgs = 1 the waves of one workgroup cross replica boundaries."""
    assert [nb for nb in range(1, 2047) if (8 + 4 * 24) * (nb + 2) <= 65536][-1] == 628
    assert [nb for nb in range(1, 2047) if (8 + 2 * 24) * (nb + 2) <= 65536][-1] == 1168
    assert (8 + 24) * (2046 + 2) <= 65536 < (8 + 24) * (2047 + 2)
    box = 22.0
    a = small_system(129, box, seed=229)
    with make_batch(a, 3) as b:
        want = want_rows(b, [box] * 3, numbins)
        for wgs in (1, 0):
            b.set_option("wave_wgs", wgs)
            check_batch(b, [box] * 3, numbins, what=f"{numbins} bins, wave_wgs {wgs}", want=want)


def per_box_states(factors):
    a = common.nist_arrays(4, "unwrapped")
    out = []
    for f in factors:
        com = a["com"] * f
        out.append(dict(a, com=com, coords=a["coords"] + np.repeat(com - a["com"], 3, axis=0),
                        box=float(a["box"] * f)))
    return out


def per_box_batch(states):
    from metropolismontecarlo_amd.device import Batch
    a0 = states[0]
    b = Batch(len(states), a0["com"], a0["coords"], a0["atype"], a0["charge"], a0["eps"], a0["sig"],
              a0["box"], ALPHA / a0["box"], structs.factor, RCUT, RCUT)
    for r, a in enumerate(states):
        b.set_replica(r, a["com"], a["coords"])
    b.set_boxes([a["box"] for a in states], ALPHA)
    b.recip_long()
    return b


def check_dipoles(b, charge, boxes):
    d = b.dipoles()
    assert d.shape == (b.R, 3)
    assert np.array_equal(d, b.dipoles())                       # identical bits, run to run
    for r in range(b.R):
        com, coords, _ = b.get_replica(r)
        mu = ref.molecule_dipoles(com, coords, charge, float(boxes[r]))
        assert np.all(np.abs(d[r] - mu.sum(0)) <= 1e-12 * np.abs(mu).sum(0)), r
    return d


def test_per_replica_boxes():
    states = per_box_states([0.97, 1.0, 1.04])
    with per_box_batch(states) as b:
        boxes = b.get_boxes()
        check_batch(b, boxes, 60, r_max=RCUT, what="per box")
        check_dipoles(b, states[0]["charge"], boxes)
        e0 = b.potential_ewald(as_array=True)["energy"].copy()
        b.run_npt_replicas(2, T, 0.0024, 300.0, DR, DPHI, seed=9, energies=e0, moves_per_sweep=40)
        boxes = b.get_boxes()
        check_batch(b, boxes, 60, r_max=RCUT, what="per box, after sweeps")
        check_batch(b, boxes, 33, r_max=0.5 * boxes.min(), what="per box, half the smallest box")
        check_dipoles(b, states[0]["charge"], boxes)
        out = np.full((6, 11), 77, dtype=np.uint64)
        for r_max in (0.0, -1.0, np.nextafter(0.5 * boxes.min(), 100.0), 0.5 * boxes.max()):
            with pytest.raises(_lib.MMCError) as ei:
                b.rdf_sites(10, r_max, out=out)
            assert ei.value.status == _lib.MMC_ERR_ARG and np.all(out == 77), r_max


def test_launch_shape_does_not_change_the_counts():
    a = common.nist_arrays(4, "unwrapped")
    n_cus = common.device_cu_count()
    tiles = 12 * 13 // 2                                   # 750 molecules: K = 12 blocks
    R = -(-3 * 16 * n_cus // tiles) + 1                    # > 3 tiles per wave of the default grid
    with make_batch(a, R) as b:
        b.set_option("device_moves", 1)
        b.run(40, T, DR, DPHI, seed=11)
        base_per = b.rdf_sites(120, RCUT, per_replica=True)
        base_tot = b.rdf_sites(120, RCUT)
        assert np.array_equal(base_per.sum(0), base_tot)
        boxes = [a["box"]] * R
        for r in sorted({0, 1, R // 2, R - 1}):            # a few replicas against the restatement
            want = ref.six_rows(b.get_replica(r)[1], boxes[r], 120, RCUT)
            assert np.array_equal(base_per[r], want), r
        d0 = b.dipoles()
        for wgs in (1, 3, 64):
            b.set_option("wave_wgs", wgs)
            assert np.array_equal(b.rdf_sites(120, RCUT, per_replica=True), base_per), wgs
            assert np.array_equal(b.rdf_sites(120, RCUT), base_tot), wgs
            assert np.array_equal(b.dipoles(), d0), wgs
        b.set_option("wave_wgs", 0)
    with make_batch(a, 1) as b1:
        for wgs in (0, 1, 5):
            b1.set_option("wave_wgs", wgs)
            check_batch(b1, [a["box"]], 120, RCUT, what=f"R = 1, wave_wgs {wgs}")


@pytest.mark.parametrize("k", [1, 4])
def test_dipoles_against_numpy_and_both_com_conventions(k):
    au, ar = common.nist_arrays(k, "unwrapped"), common.nist_arrays(k, "reference")
    with make_batch(au, 2) as bu, make_batch(ar, 2) as br:
        du = check_dipoles(bu, au["charge"], [au["box"]] * 2)
        dr_ = check_dipoles(br, ar["charge"], [ar["box"]] * 2)
        scale = np.abs(ref.molecule_dipoles(au["com"], au["coords"], au["charge"], au["box"])).sum(0)
        for r in range(2):
            assert np.all(np.abs(du[r] - dr_[r]) <= 1e-12 * scale), r
        assert np.abs(du).max() > 0.1                           # e A: not a vanishing sum
        bu.run(120, T, DR, DPHI, seed=3, n_groups=1)
        check_dipoles(bu, au["charge"], [au["box"]] * 2)


def chain(b, interleave, n_blocks=3, steps=70, npt=False):
    e = b.potential_ewald(as_array=True)["energy"].copy()
    stats = []
    for blk in range(n_blocks):
        if interleave:
            b.rdf_sites(50, RCUT, per_replica=bool(blk & 1))
            b.dipoles()
        if npt:
            e, st, _ = b.run_npt_replicas(1, T, 0.0024, 300.0, DR, DPHI, seed=21, energies=e, moves_per_sweep=steps)
        else:
            e, st = b.run(steps, T, DR, DPHI, seed=21, energies=e)
        stats.append({k: v for k, v in st.items() if isinstance(v, int)})
    if interleave:
        b.rdf_sites(50, RCUT)
        b.dipoles()
    return e, stats, [b.get_replica(r) for r in range(b.R)]


def same_chain(x, y):
    assert np.array_equal(x[0], y[0])
    assert x[1] == y[1]
    for p, q in zip(x[2], y[2]):
        assert all(np.array_equal(u, v) for u, v in zip(p, q))


def test_calls_between_blocks_leave_the_chain_bit_identical():
    a = common.nist_arrays(4, "unwrapped")
    runs = []
    for interleave in (False, True):
        with make_batch(a, 6) as b:                              # default options: the wave kernel decides
            b.set_option("device_moves", 1)
            runs.append(chain(b, interleave))
    same_chain(*runs)
    runs = []
    for interleave in (False, True):
        with per_box_batch(per_box_states([0.98, 1.03])) as b:
            runs.append(chain(b, interleave, npt=True) + (b.get_boxes(),))
    same_chain(runs[0][:3], runs[1][:3])
    assert np.array_equal(runs[0][3], runs[1][3])


def test_refusals_leave_outputs_untouched():
    a = common.nist_arrays(1, "unwrapped")
    R = 2
    L = _lib.lib()

    def expect(status, b, numbins=10, r_max=0.0, per=False):
        h = np.full((R, 6, max(numbins, 0) + 1) if per else (6, max(numbins, 0) + 1), 99, dtype=np.uint64)
        with pytest.raises(_lib.MMCError) as ei:
            b.rdf_sites(numbins, r_max, per_replica=per, out=h)
        assert ei.value.status == status and np.all(h == 99)

    def expect_dip(status, b):
        d = np.full((R, 3), 7.5)
        with pytest.raises(_lib.MMCError) as ei:
            b.dipoles(out=d)
        assert ei.value.status == status and np.all(d == 7.5)

    with make_batch(a, R) as b:
        # proposals outstanding
        com, coords = np.asarray(a["com"]), np.asarray(a["coords"])
        b.eval(np.full(R, 3), np.tile(com[2], (R, 1)), np.tile(coords[6:9], (R, 1, 1)))
        expect(_lib.MMC_ERR_STATE, b)
        expect(_lib.MMC_ERR_STATE, b, per=True)
        expect_dip(_lib.MMC_ERR_STATE, b)
        b.settle(np.zeros(R, dtype=np.int32))
        # bad arguments
        for nb in (0, -3):
            expect(_lib.MMC_ERR_ARG, b, numbins=nb)
        for r_max in (float("nan"), float("inf"), -float("inf"), np.nextafter(a["box"] / 2, 100.0)):
            expect(_lib.MMC_ERR_ARG, b, r_max=r_max)
            expect(_lib.MMC_ERR_ARG, b, r_max=r_max, per=True)
        expect(_lib.MMC_ERR_ARG, b, numbins=2047)          # above what one wave's histograms may take of the LDS
        assert L.mmc_batch_rdf_sites(b._h, 10, 0.0, 0, None) == _lib.MMC_ERR_ARG
        assert L.mmc_batch_dipoles(b._h, None) == _lib.MMC_ERR_ARG
        # ... and after all that the calls work, r_max = L / 2 exactly included
        assert np.array_equal(b.rdf_sites(10, a["box"] / 2), b.rdf_sites(10))
        assert b.dipoles().shape == (R, 3)
    # a volume trial in flight
    with per_box_batch(per_box_states([1.0, 1.02])) as b:
        boxes = b.get_boxes()
        b.volume_trial_replicas(boxes * np.array([1.01, 0.0]))
        expect(_lib.MMC_ERR_STATE, b, r_max=RCUT)
        expect_dip(_lib.MMC_ERR_STATE, b)
        b.volume_settle(np.zeros(R, dtype=np.int32))
        assert b.rdf_sites(10, RCUT).sum() > 0

