"""The device's own sine / cosine (sincos_moderate, csrc/mmc_device.hpp) and the integer powers the
kernels build from it, read through S(k) and held to exact references.

A replica of ONE molecule with charges (1, 0, 0) exposes single phase factors: S(k) for k = (1,0,0)
is (cos, sin) of MMC_TWOPI x / L of the charged atom with no rounding in between -- the charge is
1, the other factors are (1, 0), the uncharged atoms and the idle lanes add zeros -- (0,1,0) and
(0,0,1) give the same for y and z, and (n,0,0), (0,n,0), (0,0,n), n = 2..5, the powers made by
repeated c_mul (ewalds.jl:575-585).  One replica carries three arguments.  Of a conjugate pair of the
kx = 0 plane the batch computes one member, (0,-n,0) and (0,0,-n) (elementary_ref.stored_axis_vectors),
and copies the other: the computed one is read.

Every entry is compared with tests/elementary_ref.py BIT FOR BIT (the library is built with
-ffp-contract=off and sincos_moderate spells out its fma), and every n = 1 entry, independently of
that restatement, with 50-digit mpmath at the accuracy mmc_device.hpp documents
(elementary_ref.error_bound).  If the bits differ the failure says whether the first power (the
argument or sincos_moderate) or only the recurrence is off; it is not to be loosened into a
tolerance.

Arguments: families A, B, C and E of elementary_ref (coordinates within a few box lengths, quadrant
edges, up to 1e5 box lengths, tiny and subnormal) in the boxes 20, 30 and 32 on every path that
calls sincos_moderate for RecipLong; family D (the fold-back branch, |argument| from 8e5 to 1e9) on
one; the move kernels' phase_row_moderate through one accepted translation."""
import math

import numpy as np
import pytest

import elementary_ref as er

pytestmark = pytest.mark.gpu

RCUT = 10.0
SEED = 20261021
OTHER_ATOMS = ((1.25, 17.5, 6.0625), (-3.5, 0.3, 41.0))   # the two uncharged atoms: anywhere
KV = er.kvectors()
KINDEX = {k: i for i, k in enumerate(KV)}


# ---- arguments and their references, made once ---------------------------------------------------
def _chunks3(xs):
    xs = list(xs)
    while len(xs) % 3:
        xs.append(xs[len(xs) % 7])        # (pad the last replica with arguments already in the list)
    return [tuple(xs[i:i + 3]) for i in range(0, len(xs), 3)]


@pytest.fixture(scope="module")
def main_replicas():
    """{L: [(x, y, z) ...]}: families A, B, C, E as positions of the charged atom, per box."""
    rng = np.random.default_rng(SEED)
    out = {}
    for L in er.BOXES:
        xs = er.family_a(L, 400, rng) + er.family_c(L, 400, rng) + er.family_e(L, 90, rng)
        if L == 20.0:
            xs += er.family_b(L)
        if L == 32.0:
            xs += er.family_b_fractions(L)
        assert all(er.in_main_branch(er.argument(x, L)) for x in xs)
        out[L] = _chunks3(xs)
    return out


@pytest.fixture(scope="module")
def fold_replicas():
    rng = np.random.default_rng(SEED + 1)
    return {L: _chunks3(er.family_d(L, 250, rng)) for L in er.BOXES}


class Reference:
    """Restated phases and mpmath errors of every argument seen, computed once for all tests."""

    def __init__(self):
        self._phase, self._exact = {}, {}

    def phase(self, x, L):
        key = (float(x).hex(), L)
        if key not in self._phase:
            self._phase[key] = er.phase(x, L)
        return self._phase[key]

    def exact(self, arg):
        key = float(arg).hex()
        if key not in self._exact:
            self._exact[key] = er.exact(arg)
        return self._exact[key]


@pytest.fixture(scope="module")
def ref():
    return Reference()


def _coords(xyz):
    return np.array([xyz, OTHER_ATOMS[0], OTHER_ATOMS[1]], dtype=float)


def _system(L):
    """What Batch / Context need besides coordinates: one molecule of three sites, one atom type
    without LJ, charges (1, 0, 0)."""
    return dict(atype=np.ones(3, dtype=np.int64), charge=np.array([1.0, 0.0, 0.0]),
                eps=np.zeros((1, 1)), sig=np.ones((1, 1)), box=float(L))


def make_batch(L, R, xyz):
    from metropolismontecarlo_amd import structs
    from metropolismontecarlo_amd.device import Batch
    a = _system(L)
    return Batch(R, np.zeros((1, 3)), _coords(xyz), a["atype"], a["charge"], a["eps"], a["sig"], L,
                 5.6 / L, structs.factor, RCUT, RCUT)


def _same_bits(a, b):
    return float(a).hex() == float(b).hex()


class Findings:
    """Collects every disagreement of a path (no argument is skipped, none stops the others)."""

    def __init__(self, path):
        self.path, self.bits, self.mp, self.n_args, self.worst = path, [], [], 0, 0.0

    def check(self, ref, S, index, L, xyz, both_signs=False):
        """The 15 axis entries of one replica's S(k) (`index`: k -> position in S)."""
        ph = [ref.phase(c, L) for c in xyz]
        for axis in range(3):
            self.n_args += 1
            first_power_off = False
            for n, k in er.stored_axis_vectors(axis):
                ks = [k, tuple(-c for c in k)] if both_signs and axis > 0 else [k]
                for kk in ks:
                    got = S[index[kk]]
                    want = er.single_atom_S(kk, *ph)
                    if not (_same_bits(got.real, want[0]) and _same_bits(got.imag, want[1])):
                        first_power_off = first_power_off or n == 1
                        what = ("first power: the argument or sincos_moderate" if n == 1 else
                                "follows the first power" if first_power_off else
                                "the recurrence alone (c_mul): the first power agrees")
                        self.bits.append((L, xyz[axis], kk, (float(got.real).hex(), float(got.imag).hex()),
                                          (want[0].hex(), want[1].hex()), what))
                if n == 1:      # against mpmath, whatever the restatement says
                    got = S[index[k]]
                    arg = er.argument(xyz[axis], L)
                    cs, sn = got.real, (got.imag if k[axis] > 0 else -got.imag)
                    es, ec = ref.exact(arg)
                    err = max(er.abs_error(sn, es), er.abs_error(cs, ec))
                    bound = er.error_bound(arg)
                    if er.in_main_branch(arg):
                        self.worst = max(self.worst, float(err))
                    if not err <= bound:
                        self.mp.append((L, xyz[axis], arg, sn, cs, float(err), float(bound)))

    def assert_clean(self):
        print(f"{self.path}: {self.n_args} arguments, max |error| in the main branch "
              f"{self.worst:.4e} = {self.worst / 2.0 ** -53:.3f} x 2^-53")
        msgs = []
        if self.mp:
            fam_c = sum(abs(x) >= 10 * L for L, x, *_ in self.mp)
            msgs.append(f"{len(self.mp)} of {self.n_args} arguments outside the mpmath bound ({fam_c} of them "
                        f"coordinates beyond 10 L), e.g. (L, x, arg, sin, cos, error, bound) {self.mp[:3]}")
        if self.bits:
            first = sum(w.startswith("first power") for *_, w in self.bits)
            alone = sum(w.startswith("the recurrence alone") for *_, w in self.bits)
            msgs.append(f"{len(self.bits)} entries differ from the restatement in their bits ({first} first "
                        f"powers, {alone} powers whose first power agrees), e.g. (L, x, k, got, want, where) "
                        f"{self.bits[:3]}")
        assert not msgs, f"{self.path}: " + "; ".join(msgs)


def _run_batch_all_at_once(find, ref, L, reps, boxes=None):
    """One batch with a replica per entry of reps; S(k) of every replica checked."""
    R = len(reps)
    with make_batch(L, R, reps[0]) as b:
        for r, xyz in enumerate(reps):
            b.set_replica(r, np.zeros((1, 3)), _coords(xyz))
        if boxes is not None:
            b.set_boxes(boxes)
            assert np.array_equal(b.get_boxes(), boxes)
        b.recip_long()
        for r, xyz in enumerate(reps):
            find.check(ref, b.get_replica(r)[2], KINDEX, L if boxes is None else float(boxes[r]), xyz)


# ---- RecipLong: the paths that call sincos_moderate ----------------------------------------------
def test_recip_long_lds_kernel(main_replicas, ref):
    """k_recip_long_lds: recip_long_enqueue takes it for one shared box when 66 R >= 16384, i.e.
    R >= 249, and the replica's phases fit LDS (7 doubles x 3 atoms).  Every box's batch is larger."""
    find = Findings("k_recip_long_lds")
    for L, reps in main_replicas.items():
        assert 66 * len(reps) >= 16384, (L, len(reps))
        _run_batch_all_at_once(find, ref, L, reps)
    find.assert_clean()


def test_recip_long_atom_phases_and_column_kernels(main_replicas, ref):
    """k_atom_phases + k_recip_long_ph<256>: R = 8 (66 R < 16384, so no LDS kernel; three atoms are
    one chunk).  The arguments pass through the eight replicas in turn."""
    find = Findings("k_atom_phases, R = 8")
    R = 8
    assert 66 * R < 16384
    for L, reps in main_replicas.items():
        with make_batch(L, R, reps[0]) as b:
            for i in range(0, len(reps), R):
                group = reps[i:i + R]
                for r, xyz in enumerate(group):
                    b.set_replica(r, np.zeros((1, 3)), _coords(xyz))
                b.recip_long()
                for r, xyz in enumerate(group):
                    find.check(ref, b.get_replica(r)[2], KINDEX, L, xyz)
    find.assert_clean()


def test_recip_long_per_replica_boxes(main_replicas, ref):
    """k_atom_phases_pb (+ k_recip_long_ph<64>, 66 R >= 16384): after set_boxes with differing boxes
    recip_long_enqueue always takes the phase path, and the argument is formed with each replica's
    own box.  The batch is created in box 32 and holds the replicas of all three boxes interleaved,
    so a kernel reading the shared box would get two thirds of them wrong."""
    find = Findings("k_atom_phases_pb")
    reps, boxes = [], []
    longest = max(len(v) for v in main_replicas.values())
    for i in range(longest):
        for L, v in main_replicas.items():
            if i < len(v):
                reps.append(v[i])
                boxes.append(L)
    boxes = np.array(boxes)
    assert len(set(boxes)) == 3 and 66 * len(reps) >= 16384
    _run_batch_all_at_once(find, ref, 32.0, reps, boxes=boxes)
    find.assert_clean()


def test_recip_long_one_system_launch(main_replicas, ref):
    """k_potential_one's reciprocal workgroups: recip_long_all of a batch of R = 1 goes through
    potential_one (one launch, the phases made in registers); get_replica reads what it stored."""
    find = Findings("k_potential_one, R = 1")
    for L, reps in main_replicas.items():
        with make_batch(L, 1, reps[0]) as b:
            for xyz in reps:
                b.set_replica(0, np.zeros((1, 3)), _coords(xyz))
                b.recip_long()
                find.check(ref, b.get_replica(0)[2], KINDEX, L, xyz)
    find.assert_clean()


def test_recip_long_of_a_context(main_replicas, ref):
    """A Context: recip_long then get_sumqexp.  It keeps the reference's full k-vector list, so both
    members of the conjugate pairs of the kx = 0 plane are computed, and both are checked."""
    from metropolismontecarlo_amd import structs
    from metropolismontecarlo_amd.device import Context
    find = Findings("Context")
    for L, reps in main_replicas.items():
        a = _system(L)
        with Context() as ctx:
            ctx.upload_system(np.zeros((1, 3)), [1], [3], _coords(reps[0]), a["atype"], a["charge"], a["eps"],
                              a["sig"], L)
            assert ctx.prepare_ewald(5.6 / L, 5, 27, L, structs.factor) == len(KV)
            kxyz, _ = ctx.get_kvectors()
            assert [tuple(int(c) for c in k) for k in kxyz] == KV
            for xyz in reps:
                ctx.update_system(np.zeros((1, 3)), _coords(xyz))
                ctx.recip_long()
                s_old, s_new = ctx.get_sumqexp()
                assert np.array_equal(s_old.view(np.int64), s_new.view(np.int64))   # ewalds.jl:600-601
                find.check(ref, s_old, KINDEX, L, xyz, both_signs=True)
    find.assert_clean()


def test_fold_back_branch(fold_replicas, ref):
    """Family D, |argument| from just below 8e5 to 1e9, both signs, through k_atom_phases and the
    column kernels (R < 249).  The batch takes coordinates that far out as they are.  Bit for bit
    the restatement; against mpmath |error| <= |arg| 2^-52 + 2^-52."""
    find = Findings("fold-back, k_atom_phases")
    n_folded = 0
    for L, reps in fold_replicas.items():
        assert 66 * len(reps) < 16384
        n_folded += sum(not er.in_main_branch(er.argument(c, L)) for xyz in reps for c in xyz)
        _run_batch_all_at_once(find, ref, L, reps)
    assert n_folded > 700
    find.assert_clean()


# ---- the move kernels' phase_row_moderate ---------------------------------------------------------
def _move_bound(kernel, n):
    """What |S(k) after an accepted move - S(k) of RecipLong on the new coordinates| may be for the
    axis entry of power n, per component (see test_move_kernel_phase_rows)."""
    if kernel != 1:
        return 2 * 2.0 ** -53
    return (2 * math.sqrt(2.0) * (10 * n - 6) + 2) * 2.0 ** -53 * (1 + 2.0 ** -20)


@pytest.mark.parametrize("kernel,parts", [(2, 1), (1, 1), (4, 16)])
def test_move_kernel_phase_rows(kernel, parts, main_replicas, ref):
    """One accepted translation of the one molecule (eval + settle) in 64 replicas, then S(k) against
    recip_long() recomputed on the same coordinates, axis entries of every power n = 1..5.

    Kernels 2 and 4 (mmc_wave_unit.inc, mmc_wave_lat.inc) build the rows of the moved atoms with
    phase_row_moderate -- sincos_moderate and the same c_mul recurrence as RecipLong -- and update

        S_new = fma(q, tn - to, S_old),   tn, to = c_mul_fused(c_mul_fused(X, Y), Z)   (new, old).

    On an axis entry two of X, Y, Z are (1, 0): c_mul_fused(a, (1, 0)) = (fma(a.re, 1, -(a.im 0)),
    fma(a.re, 0, a.im 1)) = a exactly, so tn and to ARE the row entries, i.e. the bits RecipLong
    stores for the new and the old coordinates; S_old is RecipLong's, hence S_old = to bit for
    bit; q = 1, and the uncharged atoms add fma(0, ., S) = S.  What is left is fl(to + fl(tn - to))
    against tn: the subtraction has |result| <= 2, so it rounds by at most 2^-53; the sum is tn up
    to that, |sum| < 2, and rounds by at most 2^-53 again:

        |S_move - S_recip| <= 2 x 2^-53   per component, every power.

    Kernel 1 (k_move_eval_fast, mmc_fast.hpp) does NOT use phase_row_moderate: its rows come from
    phase_row, the library's sincos, with unfused products, S_new = S_old + q (tn' - to').  tn' and
    to' then differ from RecipLong's values by the two functions' errors, carried through the
    recurrence.  With d the component error of a first power (library: 2 ulp <= 2^-52, OCML's
    stated accuracy; sincos_moderate: 2^-52, test_elementary_host.py) and rho = 3 x 2^-53 the three
    roundings of a c_mul component, |p_n - z^n| <= n sqrt(2) d + (n - 1) sqrt(2) rho to first order,
    so the two versions of a row entry differ by at most sqrt(2) (10 n - 6) 2^-53, old and new alike,
    and the two roundings of the update come on top:

        |S_move - S_recip| <= (2 sqrt(2) (10 n - 6) + 2) x 2^-53   (15.7e-16 at n = 1, 1.4e-14 at n = 5).

    The recomputed S(k) is also the restatement's, bit for bit, and the coordinates are the move's."""
    L, R = 20.0, 64
    pool = [c for xyz in main_replicas[L] for c in xyz]
    rng = np.random.default_rng(SEED + kernel)
    old = [tuple(float(c) for c in rng.choice(pool, 3)) for _ in range(R)]
    new = [tuple(float(c) for c in rng.choice(pool, 3)) for _ in range(R)]
    new[0] = (0.0, L / 4, -L / 2)          # exact quadrant edges as the move's target
    old[1] = (L, 3 * L / 4, -0.0)          # ... and as its origin

    def atoms(xyz):                        # the three sites in one place: a rigid translation
        return np.tile(np.array(xyz, dtype=float), (3, 1))

    find = Findings(f"recip_long after the move, kernel {kernel}")
    worst = {n: 0.0 for n in range(1, er.NK + 1)}
    bad = []
    with make_batch(L, R, old[0]) as b:
        for r in range(R):
            b.set_replica(r, np.array([old[r]]), atoms(old[r]))
        b.set_option("kernel", kernel)
        b.set_parts(parts)
        b.recip_long()
        _, ov = b.eval(1, np.array(new), np.array([atoms(x) for x in new]))
        assert not ov.any()
        b.settle(np.ones(R, dtype=np.int32))
        moved = [b.get_replica(r) for r in range(R)]
        b.recip_long()
        for r in range(R):
            com, coords, S_move = moved[r]
            assert np.array_equal(com[0], np.array(new[r])) and np.array_equal(coords, atoms(new[r])), r
            S_ref = b.get_replica(r)[2]
            # the sites are in one place: the uncharged ones add zeros wherever they are
            find.check(ref, S_ref, KINDEX, L, new[r])
            for axis in range(3):
                for n, k in er.stored_axis_vectors(axis):
                    d = S_move[KINDEX[k]] - S_ref[KINDEX[k]]
                    err = max(abs(d.real), abs(d.imag))       # (exact: the two agree to ~2^-50)
                    worst[n] = max(worst[n], err)
                    if not err <= _move_bound(kernel, n):
                        bad.append((r, k, old[r][axis], new[r][axis], err / 2.0 ** -53))
    print(f"kernel {kernel}: max |S_move - S_recip| in units of 2^-53, n = 1..5: "
          + ", ".join(f"{worst[n] / 2.0 ** -53:.2f}" for n in worst))
    find.assert_clean()
    assert not bad, (f"kernel {kernel}: {len(bad)} axis entries beyond the bound, e.g. "
                     f"(replica, k, x_old, x_new, error / 2^-53) {bad[:5]}")
