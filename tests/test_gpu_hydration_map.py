"""mmc_batch_hydration_map on the device against tests/hydration_map_ref.py: counts and orientation sums
integer for integer, the energy channels against the oracle's per-water pair energies within one unit
of 2^-20 K per deposit, planted waters on the cube's edges and ends, independence of the launch, and
the refusals that need a batch.

The systems are test_gpu_solute_chain.py's: NIST configuration 3 (a 20 A box, a dyadic number) reduced
to 257 waters -- 4 x 64 + 1, so the fifth wave holds one water and eleven waves none; the 1024 threads
make ONE pass of their stride here (a second pass, and a thread whose tails take more than one deposit
before a flush, are test_gpu_solute_chain_shapes.py's, at 1090 waters) -- three
replicas diversified by 600 device-proposed steps and doubled to six, so that under wave_wgs = 1 one
workgroup strides over replicas; cutoffs LJ 8.5 and real space 9.5 A; the solute at corner(box), so that
the cube crosses a face, an edge and the corner of the box."""
import numpy as np
import pytest

import hydration_map_ref as hm
import solute_ref as sr
import test_gpu_solute_chain as tsc
from test_gpu_solute_chain import cfg3, diversified, orc  # noqa: F401  (fixtures)
from metropolismontecarlo_amd import _lib

pytestmark = pytest.mark.gpu

LJ, QQ, T = tsc.LJ, tsc.QQ, tsc.T
GRIDS = ((1, 0.5), (1, 10.0), (7, 0.7), (12, 0.5))
SENTINEL = -0x0123456789abcdef
_cache = {}


def ref_maps(reps, mol, box, n_half, cell, energies=None):
    """[len(reps), 8, cells + 2]: the restatement of every replica (energies: per replica (u_lj, u_real, ov))."""
    return np.array([hm.hydration_map(mol, coords, box, n_half, cell, *(energies[r] if energies else ()))
                     for r, (_, coords) in enumerate(reps)])


def oracle_energies(orc, a, reps, name, mol):
    """Per replica (u_lj, u_real, ov) [N] of the oracle, computed once per solute and placement."""
    key = (name, np.asarray(mol).tobytes(), tuple(c.tobytes() for _, c in reps))
    if key not in _cache:
        so = sr.SoluteOracle(orc, a, tsc.solute_of(name, a), LJ, QQ)
        _cache[key] = [hm.water_energies(so, com, coords, mol, float(a["box"])) for com, coords in reps]
    return _cache[key]


# ---- 1. counts and orientation ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("methane", "cation", "synthetic16"))
def test_counts_and_orientation_integer_for_integer(diversified, name):
    a, reps = diversified
    sol, box = tsc.solute_of(name, a), float(a["box"])
    mol = sr.placed(sol.offsets, tsc.corner(box), sr.rotation(np.random.default_rng(4)))
    with tsc.batch_of(a, reps * 2) as b:
        b.set_solute(sol, mol)
        for k, (n_half, cell) in enumerate(GRIDS):
            b.set_option("wave_wgs", k % 2)            # one workgroup striding over the six replicas, or one each
            want = ref_maps(reps, mol, box, n_half, cell)[:, :6]
            cells = (2 * n_half) ** 3
            per = b.hydration_map(n_half, cell, channels=63, per_replica=True)
            tot = b.hydration_map(n_half, cell, channels=("O", "H1", "H2", "px", "py", "pz"))
            assert per.shape == (6, 6, cells + 2) and tot.shape == (6, cells + 2) and per.dtype == tot.dtype == np.int64
            assert (per == np.concatenate([want, want])).all(), (n_half, cell)
            assert (tot == 2 * want.sum(0)).all(), (n_half, cell)
            assert (per[:, :3].sum(2) == 257).all() and (per[:, :, cells + 1] == 0).all()
            if (n_half, cell) == (12, 0.5):            # the case shows something: deposits inside, and outside
                inside, outside = want[:, 0, :cells].sum(), want[:, 0, cells].sum()
                print(f"{name}: {inside} O inside the (12, 0.5) cube, {outside} outside, of 3 x 257")
                assert inside > 100 and outside >= 1
            if cell == 10.0:
                assert (want[:, :3, cells] == 0).all()  # the cube that is the box holds every site


# ---- 2. energies ----------------------------------------------------------------------------------------
def check_energy_rows(got, want, n_dep, what):
    """rows 6 and 7 [2, cells + 2] against the restatement: every cell and the outside slot within
    the number of unflagged deposits in it, the flagged count exactly."""
    cells = got.shape[-1] - 2
    dev = np.abs(got[:, :cells + 1] - want[:, :cells + 1])
    print(f"{what}: largest |device - sum Q20(oracle)| of a slot = {dev.max()} units of 2^-20 K "
          f"(at most {n_dep[dev.argmax() % (cells + 1)]} allowed there), {int((n_dep > 0).sum())} slots hold deposits")
    assert (dev <= n_dep[None, :]).all(), what
    assert (got[:, cells + 1] == want[:, cells + 1]).all(), what


@pytest.mark.parametrize("name", ("methane", "cation", "synthetic16"))
def test_energy_channels_against_the_oracle(orc, diversified, name):
    a, reps = diversified
    sol, box = tsc.solute_of(name, a), float(a["box"])
    mol = tsc.clear_of_the_water(sol, reps, box, 3)
    en = oracle_energies(orc, a, reps, name, mol)
    with tsc.batch_of(a, reps) as b:
        b.set_solute(sol, mol)
        u_lj, u_real, u_ov = b.solute_energy()
        for n_half, cell in ((7, 0.7), (12, 0.5)):
            cells = (2 * n_half) ** 3
            want = ref_maps(reps, mol, box, n_half, cell, en)
            got = b.hydration_map(n_half, cell, channels=("u_lj", "u_real", "O"), per_replica=True)
            assert got.shape == (3, 3, cells + 2)
            for r, (_, coords) in enumerate(reps):
                fl = hm.flagged(*en[r])
                assert not fl.any() and not u_ov[r]
                n_dep = hm.unflagged_counts(mol, coords, box, n_half, cell, fl)
                check_energy_rows(got[r, 1:], want[r, 6:], n_dep, f"{name} ({n_half}, {cell}) replica {r}")
                assert (got[r, 1:, cells + 1] == 0).all()
                assert (got[r, 0] == want[r, 0]).all() and got[r, 0].sum() == 257
                # the sum rule: the map holds the replica's pair energy
                for row, u in ((1, u_lj[r]), (2, u_real[r])):
                    s = float(got[r, row, :cells + 1].sum()) / 2.0 ** 20
                    tol = 257 * 2.0 ** -20 + 1e-9 * max(1.0, sol.n_sites / 3.0) + 1e-13 * abs(u)
                    print(f"  {name} replica {r} row {row}: map {s!r}, solute_energy {u!r}, allowed {tol:.3g}")
                    assert abs(s - u) <= tol
            if name == "methane":
                assert (got[:, 2] == 0).all()           # an uncharged solute: u_real = 0 everywhere
            else:
                assert (got[:, 2, :cells] != 0).any()


# ---- 3. planted waters ----------------------------------------------------------------------------------
def test_planted_waters_on_edges_ends_and_flags(orc, diversified):
    a, reps = diversified
    box, n_half, cell = float(a["box"]), 4, 0.5
    sol = sr.dipole(a)
    c = np.array([19.5, 0.25, 19.75])
    mol = sr.placed(sol.offsets, c)                     # upright: the sites at c + (-0.4, 0, 0) (+) and c + (0.9, 0, 0) (-)
    com, coords = reps[0][0].copy(), reps[0][1].copy()

    def plant(i, target, anchor, atoms=None):
        """water i (or the three `atoms`, O first) moved rigidly so that its atom `anchor` lands on `target`,
        exactly, its COM inside the box"""
        at = coords[3 * i:3 * i + 3] if atoms is None else atoms
        cm = com[i] if atoms is None else atoms[0]
        d = np.asarray(target, dtype=float) - at[anchor]
        shift = -box * np.floor((cm + d) / box)
        com[i], coords[3 * i:3 * i + 3] = cm + d + shift, at + d + shift
        coords[3 * i + anchor] = np.asarray(target, dtype=float) + shift      # (dyadic numbers: no rounding)
    w_out = 6 + int(np.argmax(coords[19::3, 0] - coords[18::3, 0]))   # a water whose H1 lies > 0.5 A beyond its O in x
    assert coords[3 * w_out + 1, 0] - coords[3 * w_out, 0] > 0.5
    plant(0, c + [0.5, 0.25, 0.25], 0)                  # O exactly on an interior edge: the upper cell
    plant(1, c + [-2.0, 0.25, 0.25], 0)                 # O exactly at -n_half cell: inside
    plant(2, c + [2.0, 0.25, 0.25], 0)                  # O exactly at +n_half cell: outside
    plant(w_out, c + [1.75, 0.25, 0.25], 0)             # O inside, H1 outside
    v = np.array([0.5, 0.25, 0.125])
    o = c + [-1.75, 1.75, -1.75]
    plant(4, o, 0, atoms=np.array([o, o + v, o - v]))   # the O-H vectors cancel: no frame
    plant(5, mol[1] + [0.0, 0.5, 0.0], 1)               # H1 0.5 A from the negative site: an overlap
    planted = [(com, coords), reps[1]]

    g, cells = 2 * n_half, (2 * n_half) ** 3
    sl = hm.slots(mol, coords, box, n_half, cell)
    assert sl[0, 0] == (5 * g + 4) * g + 4 and sl[1, 0] == (0 * g + 4) * g + 4 and sl[2, 0] == cells
    assert sl[w_out, 0] == (7 * g + 4) * g + 4 and sl[w_out, 1] == cells
    assert sl[4, 0] < cells and not hm.bisector(coords, box)[1][4]
    en = oracle_energies(orc, a, planted, "dipole", mol)
    fl = [hm.flagged(*e) for e in en]
    assert en[0][2][5] and fl[0][5] and not fl[0][4]    # the overlap is flagged, the frameless water is not
    want = ref_maps(planted, mol, box, n_half, cell, en)
    assert (want[0, 3:6, cells + 1] == 1).all() and want[0, 6, cells + 1] == want[0, 7, cells + 1] == fl[0].sum() >= 1
    with tsc.batch_of(a, planted) as b:
        b.set_solute(sol, mol)
        got = b.hydration_map(n_half, cell, per_replica=True)
    assert got.shape == (2, 8, cells + 2)
    assert (got[:, :6] == want[:, :6]).all()
    for r in range(2):
        n_dep = hm.unflagged_counts(mol, planted[r][1], box, n_half, cell, fl[r])
        check_energy_rows(got[r, 6:], want[r, 6:], n_dep, f"planted replica {r}")
    # the planted waters one by one, on the device's own rows
    assert got[0, 0, (5 * g + 4) * g + 4] >= 1 and got[0, 0, (4 * g + 4) * g + 4] == want[0, 0, (4 * g + 4) * g + 4]
    assert got[0, 0, 4 * g + 4] >= 1 and got[0, 0, cells] >= 1 and got[0, 1, cells] >= 1
    assert (got[0, 3:6, cells + 1] == 1).all() and (got[0, :3, cells + 1] == 0).all() and (got[0, :3].sum(1) == 257).all()
    assert got[0, 6, cells + 1] == got[0, 7, cells + 1] == fl[0].sum()


# ---- 4. independence of the launch ------------------------------------------------------------------------
def test_the_maps_do_not_depend_on_the_launch_or_the_channel_set(diversified):
    a, reps = diversified
    sol, box = tsc.solute_of("synthetic16", a), float(a["box"])
    mol = tsc.clear_of_the_water(sol, reps, box, 6)
    with tsc.batch_of(a, reps * 2) as b:
        b.set_solute(sol, mol)
        b.recip_long()
        for n_half, cell in ((3, 1.1), (12, 0.5)):
            b.set_option("wave_wgs", 0)
            full = b.hydration_map(n_half, cell, per_replica=True)
            assert b.hydration_map(n_half, cell, per_replica=True).tobytes() == full.tobytes()      # a second call
            tot = b.hydration_map(n_half, cell)
            assert (tot == full.sum(0)).all() and (full[:3] == full[3:]).all()
            b.set_option("wave_wgs", 1)
            assert b.hydration_map(n_half, cell, per_replica=True).tobytes() == full.tobytes()
            assert b.hydration_map(n_half, cell).tobytes() == tot.tobytes()
            for bit in range(8):
                b.set_option("wave_wgs", bit % 2)
                one = b.hydration_map(n_half, cell, channels=1 << bit, per_replica=True)
                assert one.shape == (6, 1, (2 * n_half) ** 3 + 2) and (one[:, 0] == full[:, bit]).all(), bit
                assert (b.hydration_map(n_half, cell, channels=1 << bit)[0] == tot[bit]).all(), bit
            pair = b.hydration_map(n_half, cell, channels=("pz", "u_real"))
            assert (pair == tot[[5, 7]]).all()
            assert (tot[6] != 0).any() and (tot[7] != 0).any() and (tot[3:6, :-2] != 0).any()


def test_the_call_leaves_the_chains_alone(diversified):
    a, reps = diversified
    sol, box = tsc.solute_of("cation", a), float(a["box"])
    mol = tsc.clear_of_the_water(sol, reps, box, 3)
    runs = []
    for with_call in (False, True):
        with tsc.batch_of(a, reps) as b:
            b.set_option("device_moves", 1)
            b.set_solute(sol, mol)
            e = b.potential_ewald(as_array=True)["energy"].copy()
            e, _ = b.run(40, T, 0.3, 0.2, seed=31, energies=e)
            info = b.state_info()
            if with_call:
                b.hydration_map(12, 0.5)
                b.hydration_map(2, 0.5, per_replica=True)
                assert b.state_info().s_stale == info.s_stale
            e2, _ = b.run(40, T, 0.3, 0.2, seed=32, energies=e.copy())
            runs.append((e.tobytes(), e2.tobytes(), [b.get_replica(r)[2].tobytes() for r in range(3)]))
    assert runs[0] == runs[1]


# ---- 5. refusals that need a batch ------------------------------------------------------------------------
def test_refusals_with_a_batch_leave_the_output_alone(diversified):
    a, reps = diversified
    sol, box = tsc.solute_of("methane", a), float(a["box"])
    mol = sr.placed(sol.offsets, tsc.corner(box))

    def refused(b, status_and_words, n_half, cell, **kw):
        shape = (8, (2 * n_half) ** 3 + 2)
        out = np.full((3,) + shape if kw.get("per_replica") else shape, SENTINEL, dtype=np.int64)
        with pytest.raises(_lib.MMCError, match=status_and_words):
            b.hydration_map(n_half, cell, out=out, **kw)
        assert (out == SENTINEL).all()
    with tsc.batch_of(a, reps) as b:
        b.set_solute(sol, mol)
        above = np.nextafter(box / 2, box)
        refused(b, "MMC_ERR_ARG.*second image", 1, above)
        refused(b, "MMC_ERR_ARG.*second image", 4, above / 4, per_replica=True)      # (4 * (above / 4) == above: powers of two)
        assert 4.0 * (above / 4) == above
        for n_half, cell in ((1, box / 2), (4, box / 8)):                            # exactly L / 2 passes
            m = b.hydration_map(n_half, cell, channels=7)
            assert (m[:, :-2].sum(1) == 3 * 257).all() and (m[:, -2:] == 0).all()
        # proposals outstanding
        b.eval(1, np.tile(a["com"][0], (3, 1)), np.tile(a["coords"][:3], (3, 1, 1)))
        refused(b, "MMC_ERR_STATE.*proposals outstanding", 2, 0.5)
        b.settle(np.zeros(3, dtype=np.int32))
        assert b.hydration_map(2, 0.5).shape == (8, 66)
        b.set_solute(None)
        refused(b, "MMC_ERR_STATE.*no solute", 2, 0.5)
        refused(b, "MMC_ERR_STATE.*no solute", 1, above, per_replica=True)           # the solute is asked for before the cube
