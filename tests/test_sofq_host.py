"""CPU tests of the structure-factor restatement (tests/sofq_ref.py) and of the observables helpers
built on mmc_batch_structure_factor's output.  The restatement is exact -- the device is held to it
bit for bit (test_gpu_sofq.py) -- so what is checked here is that its phase factors are
elementary_ref's, that its steps are the kernel's, and that it stays within a rounding per vector of
the independent direct form, far coordinates included.

Bound between the restatement's two forms: each half-space vector's value is rounded to a unit of
2^-24 once in each form and doubled, so two evaluations that differ by far less than a unit can
land one rounding apart per vector: |a - b| <= count[s] units per entry (count[s] / 2 half-space
vectors, each doubled)."""
import numpy as np
import pytest

import elementary_ref as er
import sofq_ref as sref
from metropolismontecarlo_amd import observables as obs

BOX = 20.0
UNIT = 2 ** 24


def test_the_library_symbol_exists():
    from metropolismontecarlo_amd import _lib
    assert "mmc_batch_structure_factor" in _lib.SIGNATURES


@pytest.mark.parametrize("n_max,half", [(1, 3), (2, 16), (5, 257), (8, 1054), (16, 8538), (32, 68532)])
def test_half_space_and_shell_counts(n_max, half):
    cols = sref.half_space_columns(n_max)
    assert sum(len(nz) for _, _, nz in cols) == half
    s, count, q = obs.structure_factor_shells(n_max, BOX)
    assert count.sum() == 2 * half and s[0] == 1 and s[-1] == n_max * n_max and np.all(count > 0)
    assert np.array_equal(q, 2.0 * np.pi * np.sqrt(s) / BOX)
    if n_max <= 8:
        brute = sref.shell_counts(n_max)
        assert brute[0] == 0 and np.array_equal(np.flatnonzero(brute), s) and np.array_equal(brute[s], count)
        assert brute[7] == 0 if n_max >= 3 else True            # 7 is no sum of three squares
    assert count.max() <= 552
    # a vector and its mirror image are never both in the half space
    seen = {(nx, ny, k) for nx, ny, nz in cols for k in nz}
    assert not any((-a, -b, -c) in seen for a, b, c in seen)


def test_the_phase_factors_are_the_restated_sincos_moderate():
    """sofq_rows takes its phase factors from elementary_ref.phase, coordinate by coordinate, in
    both argument branches: bit for bit, and numpy's cos / sin are not what it uses."""
    rng = np.random.default_rng(21)
    coords = sref.random_molecules(5, BOX, seed=2)
    far = er.family_d(BOX, 6, rng)
    coords[[0, 4, 7, 13, 14], [0, 1, 2, 0, 1]] = [far[24], far[25], far[-1], far[-3], far[0]]
    coords[2] = (0.0, -0.0, BOX / 4)
    assert sum(not er.in_main_branch(er.argument(v, BOX)) for v in coords.ravel()) == 4      # far[0]: just below 8e5
    ph = sref.phase_factors(coords, BOX)
    assert len(ph) == 3
    differs_from_numpy = 0
    for d, (re, im) in enumerate(ph):
        assert re.shape == im.shape == (3, 5) and re.dtype == im.dtype == np.float64
        for a in range(3):
            for m in range(5):
                x = float(coords[3 * m + a, d])
                want = er.phase(x, BOX)
                assert (float(re[a, m]).hex(), float(im[a, m]).hex()) == (want[0].hex(), want[1].hex()), (a, m, d)
                ang = er.argument(x, BOX)
                differs_from_numpy += (np.cos(ang), np.sin(ang)) != want
    assert differs_from_numpy > 0           # (the two are different functions: the test can tell them apart)
    # ... and sofq_rows is built on them: for ONE molecule and n_max = 1 the vectors (1,0,0), (0,1,0),
    # (0,0,1) multiply a phase factor by (1, 0) only, which is exact, so rho_a is the phase factor
    one = coords[:3]
    p1 = sref.phase_factors(one, BOX)
    rows = sref.sofq_rows(one, BOX, 1)
    for row, (a, b) in enumerate(sref.SLOT_PAIRS):
        v = [float(re[a, 0]) * float(re[b, 0]) + float(im[a, 0]) * float(im[b, 0]) for re, im in p1]
        assert rows[row, 1] == 2 * sum(int(np.rint(t * UNIT)) for t in v) and rows[row, 0] == 0, row


def test_the_product_steps_are_the_kernels():
    """The steps of sq_block (csrc/mmc_sofq.hpp) on one atom, written out with Python floats: the
    power from 1, the conjugate after the power, c_mul(xy, conj(p_k)) for -k."""
    e = [er.phase(x, BOX) for x in (3.7, 11.2, 19.9)]
    p = sref.powers((np.array([e[1][0]]), np.array([e[1][1]])), 4)
    assert (p[0][0][0], p[0][1][0]) == er.ONE
    q = er.ONE
    for k in range(1, 5):
        q = er.c_mul(q, e[1])              # sq_pow: n products from 1, the first one exact
        assert (p[k][0][0], p[k][1][0]) == q, k
    assert (p[1][0][0], p[1][1][0]) == e[1]
    # one molecule with all three sites on one point, n_max = 2: every half-space vector term by
    # term (negative ny and nz among them); all six rows are |term|^2
    coords = np.tile(np.array([[3.7, 11.2, 19.9]]), (3, 1))
    n_max = 2
    want = np.zeros(n_max * n_max + 1, dtype=np.int64)
    px, py, pz = er.powers(e[0], n_max), er.powers(e[1], n_max), er.powers(e[2], n_max)
    for nx, ny, nzs in sref.half_space_columns(n_max):
        ey = py[abs(ny)]
        if ny < 0:
            ey = er.c_conj(ey)
        xy = er.c_mul(px[nx], ey)
        for k in nzs:
            t = er.c_mul(xy, pz[k] if k >= 0 else er.c_conj(pz[-k]))
            re, im = 0.0 + t[0], 0.0 + t[1]
            want[nx * nx + ny * ny + k * k] += 2 * int(np.rint((re * re + im * im) * UNIT))
    assert np.array_equal(sref.sofq_rows(coords, BOX, n_max), np.tile(want, (6, 1)))


def test_quant_rounds_ties_to_even_as_the_magic_add_does():
    """Q on the device is (v 2^24 + 1.5 2^52) - 1.5 2^52 read as an integer: the add rounds to the
    nearest integer, ties to even.  np.rint on the same product does the same."""
    magic = 1.5 * 2.0 ** 52
    v = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999999999999994, 1234567.5, 1234568.5, -0.0, 3.0 - 2.0 ** -28,
                  2.0 ** 20 + 0.5, 2.0 ** 44 - 1.5]) * 2.0 ** -24
    by_add = ((v * sref.SCALE + magic) - magic).astype(np.int64)
    assert np.array_equal(sref.quant(v), by_add)
    assert sref.quant(v)[:6].tolist() == [0, 2, 2, 0, -2, -2]


def fp64_argument_phase_error(x, box):
    """A bound on |phase the definition uses - 2 pi x / L| (radians) for a coordinate x: the
    definition's argument is (MMC_TWOPI x) / L in fp64 -- two roundings of 2^-53 relative and the
    constant's own 2 fl(pi), 3.9e-17 relative off 2 pi: together below 2.7e-16 |arg| -- and beyond
    8e5 the periods taken off add up to |arg| 2^-52 (elementary_ref.error_bound); sincos_moderate's
    own 2^-52 comes on top."""
    arg = abs(er.argument(x, box))
    return 2.7e-16 * arg + (0.0 if er.in_main_branch(arg) else arg * 2.0 ** -52) + 2.0 ** -52


@pytest.mark.parametrize("n_mol", [1, 2])
def test_far_coordinates_stay_within_the_bound_of_the_direct_form(n_mol):
    """The fold-back branch (|argument| >= 8e5): one atom of the frame lies 2.5e6 A and more outside
    the box in every component, at the coordinates of elementary_ref.family_d that straddle the
    threshold and up to four times beyond it.

    How far out the two forms can be held to one unit per vector is not a matter of the direct
    form's argument reduction -- np.longdouble keeps 2 pi n . r / L to |arg| 2^-63, 4e-13 at 3e6,
    and its cos / sin reduce exactly -- but of the DEFINITION: it rounds the angle of a coordinate
    to fp64 before the sine is taken, and the direct form does not.  A far atom's term of vector n
    is off by at most |n|_1 times fp64_argument_phase_error (plus roundings of the products, some
    1e-15), rho_a by as much, and v_ab = rho_a . rho_b by |rho_b| <= N times that, twice in row
    (a, a).  The two forms land at most one rounding apart per vector while that stays below one
    unit of 2^-24: with ONE far atom, N <= 2 and n_max = 5 (|n|_1 <= 8) that is |argument| below
    3.8e6; the test stops at 3.2e6 and checks the figure for each of its frames.  Larger frames and
    n_max = 32 keep their coordinates within a few boxes (test_the_two_forms_agree).  Further out
    the restatement alone defines the entries, and the device is held to it bit for bit."""
    n_max = 5
    count = sref.shell_counts(n_max)
    l1 = max(nx + abs(ny) + max(abs(k) for k in nzs) for nx, ny, nzs in sref.half_space_columns(n_max))
    assert l1 == 8
    rng = np.random.default_rng(40 + n_mol)
    edge = er.family_d(BOX, 0, rng)[:26]           # +-6 ulp about the threshold, signs alternating, from below
    fars = [edge[0:3], edge[11:14], edge[23:26]]
    for _ in range(3):
        fars.append([float(s * er.FOLD_AT * f * BOX / er.TWOPI) for s, f in zip(rng.choice([-1.0, 1.0], 3), rng.uniform(1.0, 4.0, 3))])
    folded = 0
    for i, far in enumerate(fars):
        coords = sref.random_molecules(n_mol, BOX, seed=i)
        coords[1] = far                                                    # slot 1 of molecule 0
        dv = 2 * n_mol * l1 * max(fp64_argument_phase_error(v, BOX) for v in far) + 1e-14
        assert dv * UNIT < 1.0, dv * UNIT              # the two values of a vector: less than a unit apart
        folded += sum(not er.in_main_branch(er.argument(v, BOX)) for v in far)
        a, b = sref.sofq_rows(coords, BOX, n_max), sref.sofq_rows_direct(coords, BOX, n_max)
        err = np.abs(a - b)
        print(f"N {n_mol}, far atom {far}: bound on a vector's difference {dv * UNIT:.2f} units, "
              f"max |restatement - direct| = {err.max()} units")
        assert np.all(err <= count[None, :])
        assert np.all(a[:, count == 0] == 0)
    assert folded >= 12                                # (the frames below the threshold take the main branch)


@pytest.mark.parametrize("n_mol", [1, 2, 65, 129])
def test_the_two_forms_agree(n_mol):
    coords = sref.random_molecules(n_mol, BOX, seed=100 + n_mol)
    for n_max in (3, 4, 5, 6) + ((32,) if n_mol == 2 else ()):
        count = sref.shell_counts(n_max)
        a, b = sref.sofq_rows(coords, BOX, n_max), sref.sofq_rows_direct(coords, BOX, n_max)
        err = np.abs(a - b)
        print(f"N {n_mol}, n_max {n_max}: max |recurrence - direct| = {err.max()} units, bound count[s] (max {count.max()})")
        assert np.all(err <= count[None, :])
        assert np.all(a[:, count == 0] == 0) and a.dtype == np.int64 and a.shape == (6, n_max * n_max + 1)
        assert np.all(a % 2 == 0)


def test_one_molecule_and_coincident_molecules():
    n_max = 5
    count = sref.shell_counts(n_max)
    one = sref.random_molecules(1, BOX, seed=3)
    rows = sref.sofq_rows(one, BOX, n_max)
    # |e^{i phi}|^2 = 1 within an ulp or two: far less than half a unit of 2^-24
    for row in (0, 3, 5):
        assert np.array_equal(rows[row], count * UNIT)
    # 64 coincident molecules with all three sites on one point: every rho is 64 e^{i phi}, exactly
    # (one molecule per lane, and the tree adds equal numbers: powers of two times the value)
    pt = np.tile(one[:1], (3 * 64, 1))
    rows = sref.sofq_rows(pt, BOX, n_max)
    assert np.array_equal(rows, np.tile(count * (64 * 64 * UNIT), (6, 1)))


def test_a_shift_by_whole_boxes_changes_nothing_beyond_the_bound():
    n_max = 6
    count = sref.shell_counts(n_max)
    coords = sref.random_molecules(65, BOX, seed=8)
    a = sref.sofq_rows(coords, BOX, n_max)
    b = sref.sofq_rows(coords + np.array([BOX, -2 * BOX, 0.0]), BOX, n_max)
    err = np.abs(a - b)
    print(f"shift by (L, -2 L, 0): max difference {err.max()} units")
    assert np.all(err <= count[None, :])


def test_lane_sum_is_the_order_of_the_definition():
    rng = np.random.default_rng(1)
    t = rng.normal(size=200)
    lanes = np.zeros(64)
    for m in range(200):
        lanes[m % 64] = lanes[m % 64] + t[m]
    v = lanes.copy()
    for off in (32, 16, 8, 4, 2, 1):
        v[:64 - off] = v[:64 - off] + v[off:]
    assert sref.lane_sum(t) == v[0]
    assert sref.lane_sum(t[None, :])[0] == v[0]


def test_charge_and_partial_structure_factors_against_direct_sums():
    n_mol, n_max = 40, 4
    coords = sref.random_molecules(n_mol, BOX, seed=11)
    charges = np.array([-0.8476, 0.4238, 0.4238])
    rows = sref.sofq_rows(coords, BOX, n_max)
    s, count, q = obs.structure_factor_shells(n_max, BOX)
    full = np.zeros(n_max * n_max + 1, dtype=np.int64)
    full[s] = count
    # directly: every vector of every shell, both half spaces
    x = coords.reshape(n_mol, 3, 3)
    szz = np.zeros(s.size)
    soo = np.zeros(s.size)
    soh = np.zeros(s.size)
    shh = np.zeros(s.size)
    rng = range(-n_max, n_max + 1)
    for nx in rng:
        for ny in rng:
            for nz in rng:
                ss = nx * nx + ny * ny + nz * nz
                if not 0 < ss <= n_max * n_max:
                    continue
                k = int(np.searchsorted(s, ss))
                rho = np.exp(2j * np.pi * (x @ np.array([nx, ny, nz], dtype=float)) / BOX).sum(0)     # [slot]
                szz[k] += abs((charges * rho).sum()) ** 2
                soo[k] += abs(rho[0]) ** 2
                soh[k] += (rho[0] * np.conj(rho[1] + rho[2])).real
                shh[k] += abs(rho[1] + rho[2]) ** 2
    tol = 1e-5            # 2^-24 per vector and products of up to N = 40: ~1e-6 relative to N
    got = obs.charge_structure_factor(rows, full, charges, n_mol)
    assert got.shape == s.shape and np.allclose(got, szz / (n_mol * count), rtol=0, atol=tol)
    part = obs.partial_structure_factors(rows, full, n_mol, ("O", "H", "H"))
    assert set(part) == {("O", "O"), ("H", "O"), ("H", "H")}
    assert np.allclose(part[("O", "O")], soo / (n_mol * count), rtol=0, atol=tol)
    assert np.allclose(part[("H", "O")], soh / (np.sqrt(2.0) * n_mol * count), rtol=0, atol=tol)
    assert np.allclose(part[("H", "H")], shh / (2 * n_mol * count), rtol=0, atol=tol)
    # frames: two equal frames summed, as integers per replica and as the float sum
    two = np.stack([rows, rows])
    assert np.allclose(obs.charge_structure_factor(two, full, charges, n_mol), np.stack([got, got]))
    assert np.allclose(obs.charge_structure_factor(two.sum(0) / UNIT, full, charges, n_mol, n_frames=2), got)
    with pytest.raises(ValueError):
        obs.charge_structure_factor(rows[:5], full, charges, n_mol)
    with pytest.raises(ValueError):
        obs.partial_structure_factors(rows, full[:-1], n_mol, ("O", "H", "H"))


def test_dielectric_longitudinal_on_a_hand_value():
    # 4 pi * 2 * 10 * 0.5 / (1000 * 4 * 0.25) = 4 pi / 100 * ... by hand: 4 pi * 10 / 1000 = 0.04 pi
    got = obs.dielectric_longitudinal(0.5, 0.5, n_mol=10, volume=1000.0, temperature=4.0, factor=2.0)
    assert got == pytest.approx(0.04 * np.pi, rel=1e-15)
    arr = obs.dielectric_longitudinal([0.5, 2.0], [0.5, 1.0], 10, 1000.0, 4.0, 2.0)
    assert np.allclose(arr, [0.04 * np.pi, 0.04 * np.pi])
