"""The restatement of sincos_moderate (tests/elementary_ref.py) against 50-digit mpmath, on the host.

What the GPU tests (test_gpu_elementary.py) demand of the kernels bit for bit is this restatement;
here the restatement itself is held to the accuracy csrc/mmc_device.hpp documents, on the families
of arguments a coordinate x in a box L can produce (elementary_ref.family_*; boxes 20, 30 and 32):

    main branch, |arg| < 8e5:   |error| <= 2^-52               (sin and cos each)
    fold-back,   |arg| >= 8e5:  |error| <= |arg| 2^-52 + 2^-52

Maxima found (seed 20261020, absolute, the larger of sin and cos; 2^-53 = 1.11e-16 is one ulp of a
value in [0.5, 1)):

    A  x in [-3 L, 4 L]                        6000 arguments   1.5229e-16 = 1.372 x 2^-53
    B  quadrant edges and middles, +-3 ulp     3411 arguments   1.5156e-16 = 1.365 x 2^-53
    C  |x| up to 1e5 L                         6006 arguments   1.5703e-16 = 1.414 x 2^-53
    D  fold-back, |arg| up to 1e9              3084 arguments   3.853e-8, 0.350 of the bound at worst
    E  tiny and subnormal x                    3642 arguments   6.9358e-17 = 0.625 x 2^-53

so "below one ulp" does not hold (values in [0.5, 1) reach 1.4 ulp); 2^-52 does, with room.  On an
MI355X the kernels return these very bits (tests/test_gpu_elementary.py: 4131 main-branch arguments
on each of five launch paths, maximum 1.5191e-16 = 1.368 x 2^-53; 837 around and in the fold-back)."""
import math

import numpy as np
import pytest

import elementary_ref as er

SEED = 20261020


def _families():
    rng = np.random.default_rng(SEED)
    fam = {"A": [], "B": [], "C": [], "D": [], "E": []}
    for L in er.BOXES:
        fam["A"] += [(x, L) for x in er.family_a(L, 2000, rng)]
        fam["B"] += [(x, L) for x in er.family_b(L)]
        fam["C"] += [(x, L) for x in er.family_c(L, 2000, rng)]
        fam["D"] += [(x, L) for x in er.family_d(L, 1000, rng)]
        fam["E"] += [(x, L) for x in er.family_e(L, 600, rng)]
    fam["B"] += [(x, 32.0) for x in er.family_b_fractions(32.0)]
    return fam


@pytest.fixture(scope="module")
def families():
    return _families()


def _check(pairs):
    """(largest error, largest error / bound, count) over the (x, L) pairs; every one asserted."""
    worst = worst_ratio = 0.0
    for x, L in pairs:
        arg = er.argument(x, L)
        sn, cs = er.sincos_moderate(arg)
        err, bound = er.worst_error(arg, sn, cs)
        assert err <= bound, (x, L, arg, sn, cs, float(err), float(bound))
        worst, worst_ratio = max(worst, float(err)), max(worst_ratio, float(err / bound))
    return worst, worst_ratio, len(pairs)


@pytest.mark.parametrize("name", ["A", "B", "C", "E"])
def test_main_branch_within_two_to_the_minus_52(name, families):
    pairs = families[name]
    assert all(er.in_main_branch(er.argument(x, L)) for x, L in pairs)
    worst, _, n = _check(pairs)
    print(f"family {name}: {n} arguments, max |error| {worst:.4e} = {worst / 2.0 ** -53:.3f} x 2^-53")
    assert worst <= er.MAIN_BOUND
    if name != "E":   # the families are not so tame that the bound is idle: above one ulp of [0.5, 1)
        assert worst > er.ULP_HALF_TO_ONE


def test_fold_back_branch_within_its_bound(families):
    """|arg| >= 8e5: x loses n = rint(arg / 2 pi) periods of fl(2 pi), each wrong by 2 pi - fl(2 pi)
    = 2.4e-16, so the angle is off by up to n 2.4e-16 = |arg| 3.9e-17 < |arg| 2^-52 before the main
    branch adds its own 2^-52.  The family straddles the threshold: some of it is the main branch."""
    pairs = families["D"]
    folded = [(x, L) for x, L in pairs if not er.in_main_branch(er.argument(x, L))]
    below = [(x, L) for x, L in pairs if er.in_main_branch(er.argument(x, L))]
    assert len(below) >= 6 and len(folded) >= len(pairs) - 60
    args = [abs(er.argument(x, L)) for x, L in folded]
    assert min(args) == er.FOLD_AT and max(args) > 0.999e9 and max(args) <= 1.0e9
    worst, ratio, n = _check(pairs)
    print(f"family D: {n} arguments ({len(folded)} folded), max |error| {worst:.3e}, "
          f"at most {ratio:.3f} of the bound")
    assert worst > 1e-9          # the branch really costs accuracy: the bound is not the main one


def test_family_b_lands_on_the_quadrant_edges(families):
    """Family B's coordinates reach the targets themselves or stop within 4 ulp of them, on both
    sides (2 pi x and the division by L each round: consecutive coordinates land up to 4 ulp apart),
    so the reduced angle r takes both signs around every edge."""
    for L in er.BOXES:
        args = {er.argument(x, L) for x in er.family_b(L)}
        for t in er.family_b_targets():
            if t == 0.0:
                assert 0.0 in args
                continue
            lo, hi = er._ulps(t, -4), er._ulps(t, 4)
            assert any(a <= t and a >= lo for a in args) and any(a >= t and a <= hi for a in args), (L, t)
    fr = [er.argument(x, 32.0) for x in er.family_b_fractions(32.0)]
    assert fr[0] == 0.0 and math.copysign(1.0, fr[1]) < 0 and fr[2] == er.TWOPI / 4 and fr[6] == er.TWOPI


def test_special_values_of_the_restatement():
    assert er.sincos_moderate(0.0) == (0.0, 1.0)
    sn, cs = er.sincos_moderate(-0.0)   # r = fma(+0, pio2_1, -0) = +0: the sign of a zero angle is lost
    assert sn == 0.0 and math.copysign(1.0, sn) > 0 and cs == 1.0
    assert er.sincos_moderate(5e-324) == (5e-324, 1.0)
    # fma: one rounding where two differ, and the zeros
    assert er.fma(1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30, -1.0) == 2.0 ** -29 + 2.0 ** -60
    assert (1.0 + 2.0 ** -30) * (1.0 + 2.0 ** -30) - 1.0 == 2.0 ** -29
    assert math.copysign(1.0, er.fma(-0.0, 1.0, -0.0)) < 0 and math.copysign(1.0, er.fma(-0.0, 1.0, 0.0)) > 0
    assert math.copysign(1.0, er.fma(-1.0, 1.0, 1.0)) > 0
    assert er.rint(2.5) == 2.0 and er.rint(-3.5) == -4.0 and math.copysign(1.0, er.rint(-0.3)) < 0
    # the recurrence and the table of negative powers
    e1 = er.phase(3.7, 20.0)
    pw = er.powers(e1)
    assert pw[0] == er.ONE and pw[1] == e1 and pw[3] == er.c_mul(er.c_mul(e1, e1), e1)
    assert er.signed_power(pw, -2) == (pw[2][0], -pw[2][1])
    kv = er.kvectors()
    assert len(kv) == 337 and kv[0] == (0, -5, -1) and len(set(kv)) == 337
    for axis in range(3):
        assert all(k in kv for _, k in er.stored_axis_vectors(axis))
