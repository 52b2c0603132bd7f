"""CPU tests of the structure-factor restatement (tests/sofq_ref.py) and of the observables helpers
built on mmc_batch_structure_factor's output.

Bound between the restatement's two forms: each half-space vector's value is rounded to a unit of
2^-24 once in each form and doubled, so two evaluations that differ by far less than a unit can
land one rounding apart per vector: |a - b| <= count[s] units per entry (count[s] / 2 half-space
vectors, each doubled)."""
import numpy as np
import pytest

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


@pytest.mark.parametrize("n_mol", [1, 2, 65, 129])
def test_the_two_forms_agree(n_mol):
    coords = sref.random_molecules(n_mol, BOX, seed=100 + n_mol)
    for n_max in (3, 4, 5, 6):
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
