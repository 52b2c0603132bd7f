"""mmc_batch_structure_factor against its numpy restatement (tests/sofq_ref.py) on SPC/E molecules of
the NIST fixtures, truncated to the sizes at which k_sofq_wave takes another path.

Launch shape: a workgroup holds a replica's phases in LDS and its eight waves take (nx, ny) columns
from a queue; lane = molecule, so N = 63, 64, 65, 129 are a partial pass, a full one, a second pass
of one lane and a third.  |nz| is walked in blocks of 16: n_max = 32 takes three blocks, the last of
one value.  With fewer replicas than compute units `split` workgroups share a replica's columns;
with more, a persistent workgroup takes replicas g, g + G, ...; option wave_wgs sets G.  The host
walks the replicas in chunks of SQ_CHUNK_BYTES / (48 (n_max^2 + 1)): 5456 at n_max = 32
(test_replicas_beyond_one_chunk, test_last_chunk_of_one_replica_takes_the_split_regime), and
`split` changes at R = compute units / 2 (test_the_boundary_between_shared_and_whole_replicas).

No bounds: count is exact, and every per-replica entry is EQUAL to the restatement, which states
every operation of the definition (phase factors by elementary_ref's sincos_moderate, powers, sums
in lane order, Q); the summed output is host_sum of the per-replica integers byte for byte.  A
difference is a finding about the kernel or the restatement, not something to widen into a
tolerance: check_against prints its size first."""
import os
import re

import numpy as np
import pytest

import common
import elementary_ref as er
import sofq_ref as sref
from metropolismontecarlo_amd import _lib, structs
from metropolismontecarlo_amd import observables as obs

pytestmark = pytest.mark.gpu

RCUT = 9.0                      # below L / 2 = 10 of the 20 A fixtures
RCUT_PB = 10.0                  # per-replica boxes: the erfc table covers kappa = alpha / (2 r_cut) from here
T, ALPHA = 298.15, 5.6
UNIT = 2 ** 24
SIZES = (1, 2, 63, 64, 65, 129)
SENTINEL = -0x0123456789abcdef

_counts = {}


def counts(n_max):
    """count[s] by brute force, once per n_max."""
    if n_max not in _counts:
        s, c, _ = obs.structure_factor_shells(n_max, 1.0)
        full = np.zeros(n_max * n_max + 1, dtype=np.int64)
        full[s] = c
        if n_max <= 7:
            assert np.array_equal(full, sref.shell_counts(n_max))
        _counts[n_max] = full
    return _counts[n_max]


def truncated(n_mol):
    """The first n_mol molecules of NIST configuration 1 (100 molecules) or 2 (200), L = 20 A."""
    a = common.nist_arrays(1 if n_mol <= 100 else 2, "unwrapped")
    return dict(a, com=a["com"][:n_mol], coords=a["coords"][:3 * n_mol], atype=a["atype"][:3 * n_mol],
                charge=a["charge"][:3 * n_mol])


def make_batch(a, R, rcut=RCUT):
    from metropolismontecarlo_amd.device import Batch
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
              ALPHA / a["box"], structs.factor, rcut, rcut)
    b.recip_long()
    return b


def turned(a, rng):
    """(com, coords) of the frame with each molecule turned rigidly about its centre of mass by a
    random rotation and shifted by up to 0.4 A (as tests/test_gpu_orient.py)."""
    n = a["com"].shape[0]
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    w, x, y, z = q.T
    rot = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                    [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                    [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]).transpose(2, 0, 1)
    off = a["coords"].reshape(n, 3, 3) - a["com"][:, None, :]
    com = a["com"] + (rng.random((n, 3)) - 0.5) * 0.8
    coords = com[:, None, :] + np.einsum("nij,naj->nai", rot, off)
    return com, coords.reshape(-1, 3)


def diversify(b, a, seed):
    """Every replica but the first gets its own configuration (turned)."""
    rng = np.random.default_rng(seed)
    for r in range(1, b.R):
        b.set_replica(r, *turned(a, rng))


_rows = {}


def rows_of(coords, box, n_max):
    """sref.sofq_rows, once per (coordinates, box, n_max): the tests share frames (read-only)."""
    key = (np.ascontiguousarray(coords, dtype=np.float64).tobytes(), float(box), n_max)
    if key not in _rows:
        _rows[key] = sref.sofq_rows(coords, float(box), n_max)
        _rows[key].setflags(write=False)
    return _rows[key]


def want_rows(b, boxes, n_max, replicas=None):
    """[R, 6, n_max^2 + 1] from the batch's own coordinates, each replica at its box (`replicas`:
    only those, in that order)."""
    return np.stack([rows_of(b.get_replica(r)[1], boxes[r], n_max) for r in (range(b.R) if replicas is None else replicas)])


def sq_chunk(n_max):
    """Replicas per launch of mmc_batch_structure_factor (csrc/mmc_sofq.inc): SQ_CHUNK_BYTES of
    scratch over the 6 (n_max^2 + 1) 64-bit integers of a replica, the constant read from the source."""
    src = open(os.path.join(common.HERE, "..", "metropolismontecarlo_amd", "csrc", "mmc_sofq.inc")).read()
    m = re.search(r"#define SQ_CHUNK_BYTES \(\(size_t\)(\d+) << (\d+)\)", src)
    return (int(m.group(1)) << int(m.group(2))) // (48 * (n_max * n_max + 1))


def host_sum(per):
    """sq_sum as the header defines it: replicas ascending, (double)sq 2^-24, added in fp64."""
    acc = np.zeros(per.shape[1:], dtype=np.float64)
    for r in range(per.shape[0]):
        acc = acc + per[r].astype(np.float64) * 2.0 ** -24
    return acc


def check_against(b, want, n_max, what, summed=True):
    cnt = counts(n_max)
    count, per = b.structure_factor(n_max, per_replica=True)
    assert count.dtype == np.int32 and np.array_equal(count, cnt), (what, "count")
    assert per.dtype == np.int64 and per.shape == want.shape, what
    err = np.abs(per - want)
    print(f"{what}: max |device - restatement| = {err.max()} units in {np.count_nonzero(err)} of {err.size} entries")
    assert np.array_equal(per, want), (what, int(err.max()))
    assert np.all(per[:, :, cnt == 0] == 0), (what, "empty shells and s = 0")
    if summed:
        count2, tot = b.structure_factor(n_max)
        assert np.array_equal(count2, cnt) and tot.dtype == np.float64 and tot.shape == want.shape[1:], what
        assert tot.tobytes() == host_sum(per).tobytes(), (what, "summed output")
    return per


@pytest.mark.parametrize("n_mol", SIZES)
def test_against_the_restatement(n_mol):
    a = truncated(n_mol)
    box, R = a["box"], 3
    with make_batch(a, R) as b:
        diversify(b, a, seed=60 + n_mol)
        if n_mol == 65:
            # replica 2: 28 coordinates about and in sincos_moderate's fold-back branch (|argument| an
            # ulp either side of 8e5 and on to 1e9, both signs), in both passes of the lanes
            com, coords, _ = b.get_replica(2)
            far = er.family_d(box, 20, np.random.default_rng(65))
            far = far[10:16] + far[26:]
            rng = np.random.default_rng(66)
            coords.reshape(-1)[rng.choice(coords.size - 9, len(far) - 3, replace=False)] = far[3:]
            coords[3 * 64] = far[:3]                                        # molecule 64: lane 0's second
            assert sum(not er.in_main_branch(er.argument(v, box)) for v in coords.ravel()) >= 24
            b.set_replica(2, com, coords)
            assert b.get_replica(2)[1].tobytes() == coords.tobytes()
        for n_max in (1, 2, 5, 7):
            per = check_against(b, want_rows(b, [box] * R, n_max), n_max, f"N {n_mol}, n_max {n_max}")
        assert per[:, (0, 3, 5)][:, :, counts(7) > 0].min() > 0            # |rho_a|^2 > 0 in every shell that has a vector
        if n_mol > 1:
            assert not np.array_equal(per[0], per[1])


def test_molecules_that_differ_take_the_array_path():
    """A system whose molecules carry different charges has no 128-byte records: the kernel's other
    instantiation, reading the coordinate arrays."""
    box, n_mol, R = 22.0, 65, 3
    a = common.random_system(n_mol, box, seed=77, na_choices=(3,))
    with make_batch(a, R) as b:
        diversify(b, a, seed=5)
        for n_max in (2, 5):
            check_against(b, want_rows(b, [box] * R, n_max), n_max, f"ragged charges, n_max {n_max}")


def test_the_full_range():
    """n_max = 32: every block of |nz|, 68532 half-space vectors."""
    a = truncated(2)
    with make_batch(a, 2) as b:
        diversify(b, a, seed=2)
        assert counts(32).sum() == 2 * 68532
        check_against(b, want_rows(b, [a["box"]] * 2, 32), 32, "N 2, n_max 32")


def test_known_answers():
    n_max = 5
    cnt = counts(n_max)
    a = truncated(1)
    with make_batch(a, 2) as b:
        diversify(b, a, seed=1)
        _, per = b.structure_factor(n_max, per_replica=True)
        for row in (0, 3, 5):                                   # |e^{i phi}|^2 = 1
            assert np.array_equal(per[:, row], np.tile(cnt * UNIT, (2, 1))), row
    a = truncated(64)
    with make_batch(a, 2) as b:
        # 64 copies of molecule 0: rho_a = 64 e^{i phi_a}; in replica 1 every site on one point besides
        com = np.tile(a["com"][:1], (64, 1))
        b.set_replica(0, com, np.tile(a["coords"][:3], (64, 1)))
        b.set_replica(1, com, np.tile(a["com"][:1], (192, 1)))
        _, per = b.structure_factor(n_max, per_replica=True)
        big = cnt * (64 * 64 * UNIT)
        for row in (0, 3, 5):
            assert np.array_equal(per[0, row], big), row
        assert np.array_equal(per[1], np.tile(big, (6, 1)))
        _, tot = b.structure_factor(n_max)
        assert tot.tobytes() == host_sum(per).tobytes()


def test_the_launch_does_not_change_a_bit():
    a = truncated(129)
    R, n_max, pick = 5, 5, 3
    with make_batch(a, R) as b:
        diversify(b, a, seed=9)
        base = b.structure_factor(n_max, per_replica=True)[1]
        base_tot = b.structure_factor(n_max)[1]
        assert base.tobytes() == b.structure_factor(n_max, per_replica=True)[1].tobytes()      # two calls in a row
        assert base_tot.tobytes() == b.structure_factor(n_max)[1].tobytes()
        for wgs in (1, 3):
            b.set_option("wave_wgs", wgs)      # 1: one workgroup takes every part of every replica in turn
            assert b.structure_factor(n_max, per_replica=True)[1].tobytes() == base.tobytes(), wgs
            assert b.structure_factor(n_max)[1].tobytes() == base_tot.tobytes(), wgs
        com, coords, _ = b.get_replica(pick)
    with make_batch(a, 1) as b1:                # one replica: all of its columns shared out
        b1.set_replica(0, com, coords)
        for wgs in (0, 1, 3):
            b1.set_option("wave_wgs", wgs)
            assert b1.structure_factor(n_max, per_replica=True)[1][0].tobytes() == base[pick].tobytes(), wgs
            assert b1.structure_factor(n_max)[1].tobytes() == host_sum(base[pick:pick + 1]).tobytes(), wgs


def test_many_replicas_take_the_persistent_loop():
    """More replicas than compute units: one part per replica, a workgroup takes several replicas in
    turn (and with wave_wgs = 7 some forty each)."""
    a = truncated(3)
    R, n_max = 300, 3
    with make_batch(a, R) as b:
        diversify(b, a, seed=12)
        want = want_rows(b, [a["box"]] * R, n_max)
        per = check_against(b, want, n_max, f"R {R}, N 3")
        tot = b.structure_factor(n_max)[1]
        b.set_option("wave_wgs", 7)
        assert b.structure_factor(n_max, per_replica=True)[1].tobytes() == per.tobytes()
        assert b.structure_factor(n_max)[1].tobytes() == tot.tobytes()


# ---- the chunk loop (csrc/mmc_sofq.inc): sa.r0 != 0, the fetch at sq + r0 n_ent, k_sofq_reduce adding on
CHUNK_N_MAX = 32                # the smallest chunk: 256 MiB / (48 * 1025) replicas


def chunk_case():
    """(frame, chunk, five configurations of their own): two molecules at n_max = 32."""
    a = truncated(2)
    chunk = sq_chunk(CHUNK_N_MAX)
    assert chunk == 5456                                    # a changed scratch budget is noticed here
    rng = np.random.default_rng(3232)
    return a, chunk, [turned(a, rng) for _ in range(5)]


def untouched_rows_are(per, plain, touched):
    """Every row of per [R, 6, S] but `touched` equals plain [6, S]; the touched ones do not."""
    same = (per == plain[None]).all(axis=(1, 2))
    rest = np.ones(per.shape[0], dtype=bool)
    rest[list(touched)] = False
    return bool(same[rest].all()) and not same[list(touched)].any()


def test_replicas_beyond_one_chunk():
    """R = chunk + 3 = 5459 replicas: a first launch of 5456 and a second of three at r0 = 5456.
    Replicas 0, chunk - 1, chunk, chunk + 1 and R - 1 hold configurations of their own, all others the
    uploaded frame: six restatements.  Both outputs, and both again with seven persistent workgroups.

    Time on an MI355X: 25 s, nearly all of it the two wave_wgs = 7 calls -- 780 replicas in turn per
    workgroup at some 15 ms a replica of n_max = 32, 12 s a call; the two default calls take 0.3 s
    each.  Fewer molecules would not shorten it (lane = molecule: one pass of the lanes up to
    N = 64), and fewer replicas would not reach the second launch."""
    a, chunk, states = chunk_case()
    box, n_max, R = a["box"], CHUNK_N_MAX, chunk + 3
    assert R > chunk
    touched = (0, chunk - 1, chunk, chunk + 1, R - 1)
    with make_batch(a, R) as b:
        for r, (com, coords) in zip(touched, states):
            b.set_replica(r, com, coords)
        want = want_rows(b, [box] * R, n_max, touched)
        plain = rows_of(b.get_replica(chunk - 2)[1], box, n_max)
        assert b.get_replica(chunk - 2)[1].tobytes() == np.ascontiguousarray(a["coords"], dtype=np.float64).tobytes()
        count, per = b.structure_factor(n_max, per_replica=True)
        assert np.array_equal(count, counts(n_max)) and per.dtype == np.int64 and per.shape == (R, 6, n_max * n_max + 1)
        for r, w in zip(touched, want):
            err = np.abs(per[r] - w)
            print(f"replica {r}: max |device - restatement| = {err.max()} units")
            assert np.array_equal(per[r], w), (r, int(err.max()))
        assert len({w.tobytes() for w in want} | {plain.tobytes()}) == 6
        assert untouched_rows_are(per, plain, touched)
        tot = b.structure_factor(n_max)[1]
        assert tot.dtype == np.float64 and tot.tobytes() == host_sum(per).tobytes()
        b.set_option("wave_wgs", 7)
        assert np.array_equal(b.structure_factor(n_max, per_replica=True)[1], per)       # (integers: equal is the same bytes)
        assert b.structure_factor(n_max)[1].tobytes() == tot.tobytes()


def test_last_chunk_of_one_replica_takes_the_split_regime():
    """R = chunk + 1: the first launch has 5456 replicas, more than compute units, so split = 1 and
    persistent workgroups; the second has n_rep = 1, so split = min(n_cols, compute units) workgroups
    share replica `chunk`, and k_sofq_reduce adds that one replica to what the first chunk left."""
    a, chunk, states = chunk_case()
    box, n_max, R = a["box"], CHUNK_N_MAX, chunk + 1
    assert chunk >= common.device_cu_count()
    with make_batch(a, R) as b:
        b.set_replica(chunk, *states[2])
        want = rows_of(b.get_replica(chunk)[1], box, n_max)
        plain = rows_of(b.get_replica(0)[1], box, n_max)
        per = b.structure_factor(n_max, per_replica=True)[1]
        err = np.abs(per[chunk] - want)
        print(f"replica {chunk}: max |device - restatement| = {err.max()} units")
        assert np.array_equal(per[chunk], want), int(err.max())
        assert untouched_rows_are(per, plain, (chunk,))
        assert b.structure_factor(n_max)[1].tobytes() == host_sum(per).tobytes()


# ---- split = min(n_cols, cus / n_rep): where workgroups stop sharing a replica
def test_the_boundary_between_shared_and_whole_replicas():
    """N = 3.  What the host code gives, with C compute units (256 on an MI355X: the figures in
    brackets) and the 7 columns of n_max = 2 (3 of n_max = 1):
      n_max 2, R = C / 2       split 2, 2 R units, C workgroups [256]: two share a replica's columns
      n_max 2, R = C / 2 + 1   split 1, R units and workgroups [129]: a replica each
      n_max 2, R = C           split 1, C units, C workgroups [256]: one unit per workgroup
      n_max 2, R = C + 1       split 1, C + 1 units, C workgroups [256]: workgroup 0 takes a second unit
      n_max 1, R = 1           n_cols = 3 < C: split 3, 3 units, 3 workgroups (the grid is capped at
                               the units), a column each
    Every row equals the restatement, the summed output host_sum, and one workgroup doing all of it
    (wave_wgs = 1) gives the same bytes."""
    cus = common.device_cu_count()
    assert cus >= 4
    a = truncated(3)
    for n_max, R in ((2, cus // 2), (2, cus // 2 + 1), (2, cus), (2, cus + 1), (1, 1)):
        n_cols = len(sref.half_space_columns(n_max))
        assert n_cols == {2: 7, 1: 3}[n_max]
        split = max(1, min(n_cols, cus // R))
        assert split == {cus // 2: 2, 1: 3}.get(R, 1), (n_max, R)
        with make_batch(a, R) as b:
            diversify(b, a, seed=17)                                # (the same configuration in replica r of every R)
            per = check_against(b, want_rows(b, [a["box"]] * R, n_max), n_max, f"R {R}, n_max {n_max}, split {split}")
            tot = b.structure_factor(n_max)[1]
            b.set_option("wave_wgs", 1)
            assert b.structure_factor(n_max, per_replica=True)[1].tobytes() == per.tobytes(), (n_max, R)
            assert b.structure_factor(n_max)[1].tobytes() == tot.tobytes(), (n_max, R)


def test_against_the_ewald_sum():
    """The reference's reciprocal energy (Ewald/ewalds.jl:538-604 over k^2 < 27) is the charge-weighted
    sum of the shells s <= 26: factor sum_s c(s) sum_ab w_ab q_a q_b sq[ab][s] 2^-24 with
    c(s) = 2 pi exp(-b 4 pi^2 s) / (4 pi^2 s) / L, b = 1 / (4 kappa^2 L^2) (:52, :79-80), the
    undoubled coefficient.  Tolerance: half a unit of 2^-24 per half-space vector and row, doubled,
    weighted: factor sum_s c(s) count[s] (sum_a |q_a|)^2 2^-25, plus 1e-12 |E_recip| for the order
    of the energy's own sums.  n_max = 6: shell 26 = (5, 1, 0) and its like lies beyond n_max = 5,
    whose shells end at 25; the shells 27..36 of n_max = 6 get c = 0."""
    n_max, n_mol, R = 6, 129, 3
    a = truncated(n_mol)
    box = a["box"]
    q = a["charge"][:3]
    with make_batch(a, R) as b:
        diversify(b, a, seed=4)
        cnt = counts(n_max)
        _, per = b.structure_factor(n_max, per_replica=True)
        recip = b.potential_ewald(as_array=True)["recip"]
        kappa = ALPHA / box
        bb = 1.0 / 4.0 / kappa / kappa / box / box
        s = np.arange(n_max * n_max + 1, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where((s > 0) & (s <= 26), 2.0 * np.pi * np.exp(-bb * 4.0 * np.pi ** 2 * s) / (4.0 * np.pi ** 2 * s) / box, 0.0)
        w = np.array([(1.0 if i == j else 2.0) * q[i] * q[j] for i, j in obs.SLOT_PAIRS])
        tol0 = structs.factor * float((c * cnt).sum()) * float(np.abs(q).sum()) ** 2 * 2.0 ** -25
        for r in range(R):
            e = structs.factor * float((c * np.tensordot(w, per[r].astype(np.float64) * 2.0 ** -24, axes=1)).sum())
            tol = tol0 + 1e-12 * abs(recip[r])
            print(f"replica {r}: from S(q) {e!r}, RecipLong {recip[r]!r}, difference {e - recip[r]:.3e}, tolerance {tol:.3e}")
            assert abs(e - recip[r]) <= tol, r
        # ... and the helper built on the same rows
        szz = obs.charge_structure_factor(per, cnt, q, n_mol)
        assert szz.shape == (R, np.count_nonzero(cnt)) and np.all(szz >= 0)


def test_per_replica_boxes():
    a = truncated(65)
    factors = (1.0, 1.01, 1.03)
    n_max = 5
    with make_batch(a, 3, RCUT_PB) as b:
        diversify(b, a, seed=33)
        for r, f in enumerate(factors):      # every replica's own configuration, scaled to its box
            com, coords, _ = b.get_replica(r)
            b.set_replica(r, com * f, coords + np.repeat(com * f - com, 3, axis=0))
        shared = b.structure_factor(n_max, per_replica=True)[1]
        b.set_boxes([a["box"] * f for f in factors], ALPHA)
        boxes = b.get_boxes()
        per = check_against(b, want_rows(b, boxes, n_max), n_max, "per box", summed=False)
        assert np.array_equal(per[0], shared[0]) and not np.array_equal(per[2], shared[2])      # the boxes matter
        # summed over replicas: equal s are different q
        out = np.full((6, n_max * n_max + 1), -1.25)
        with pytest.raises(_lib.MMCError) as ei:
            b.structure_factor(n_max, out=out)
        assert ei.value.status == _lib.MMC_ERR_ARG and np.all(out == -1.25)


def test_wolf_style_gives_the_same_bytes():
    a = truncated(65)
    with make_batch(a, 3) as b:
        diversify(b, a, seed=6)
        per = b.structure_factor(5, per_replica=True)[1]
        tot = b.structure_factor(5)[1]
        b.set_coulomb_style("wolf")
        assert b.structure_factor(5, per_replica=True)[1].tobytes() == per.tobytes()
        assert b.structure_factor(5)[1].tobytes() == tot.tobytes()


def test_refusals_leave_outputs_untouched():
    a = truncated(65)
    R, box = 2, a["box"]

    def expect(status, b, n_max=4, per=False):
        S = max(n_max, 0) ** 2 + 1
        out = np.full((R, 6, S), SENTINEL, dtype=np.int64) if per else np.full((6, S), -1.25)
        cnt = np.full(S, -7, dtype=np.int32)
        st = _lib.lib().mmc_batch_structure_factor(
            b._h, n_max, int(per), cnt.ctypes.data_as(_lib._i32p),
            out.ctypes.data_as(_lib._i64p) if per else None, None if per else out.ctypes.data_as(_lib._dp))
        assert st == status, (n_max, per, st)
        assert np.all(cnt == -7) and np.all(out == (SENTINEL if per else -1.25)), (n_max, per)
        with pytest.raises(_lib.MMCError) as ei:
            b.structure_factor(n_max, per_replica=per, out=out)
        assert ei.value.status == status and np.all(out == (SENTINEL if per else -1.25)), (n_max, per)

    with make_batch(a, R, RCUT_PB) as b:
        # proposals outstanding
        b.eval(np.full(R, 3), np.tile(a["com"][2], (R, 1)), np.tile(a["coords"][6:9], (R, 1, 1)))
        expect(_lib.MMC_ERR_STATE, b)
        expect(_lib.MMC_ERR_STATE, b, per=True)
        expect(_lib.MMC_ERR_ARG, b, n_max=0)                      # arguments come before the state
        expect(_lib.MMC_ERR_ARG, b, n_max=33, per=True)
        b.settle(np.zeros(R, dtype=np.int32))
        assert np.array_equal(b.structure_factor(4)[0], counts(4))
        # a volume trial in flight
        b.set_boxes([box, 1.02 * box], ALPHA)
        boxes = b.get_boxes()
        b.volume_trial_replicas(boxes * np.array([1.01, 0.0]))
        expect(_lib.MMC_ERR_STATE, b, per=True)
        expect(_lib.MMC_ERR_ARG, b)                               # summed with per-replica boxes: an argument
        b.volume_settle(np.zeros(R, dtype=np.int32))
        assert np.array_equal(b.structure_factor(4, per_replica=True)[0], counts(4))


def test_too_many_molecules_are_refused():
    n_mol, box = 1025, 36.0
    a = common.random_system(n_mol, box, seed=3, na_choices=(3,))
    with make_batch(a, 1) as b:
        for per in (False, True):
            out = np.full((1, 6, 17), SENTINEL, dtype=np.int64) if per else np.full((6, 17), -1.25)
            with pytest.raises(_lib.MMCError) as ei:
                b.structure_factor(4, per_replica=per, out=out)
            assert ei.value.status == _lib.MMC_ERR_UNSUPPORTED and np.all(out == (SENTINEL if per else -1.25))


def test_the_largest_system_runs():
    """N = 1024: 147456 bytes of phases, the dynamic LDS a workgroup has to opt in for."""
    n_mol, box, n_max = 1024, 36.0, 3
    a = common.random_system(n_mol, box, seed=4, na_choices=(3,))
    with make_batch(a, 1) as b:
        check_against(b, want_rows(b, [box], n_max), n_max, "N 1024")


def test_the_call_is_read_only():
    a = truncated(64)
    R = 4
    twins = [make_batch(a, R), make_batch(a, R)]
    chains = []
    for b in twins:
        diversify(b, a, seed=14)
        b.recip_long()
        b.set_option("device_moves", 1)
        chains.append(b.new_chains(b.potential_ewald(as_array=True)["energy"]))
    b = twins[0]
    before = [b.get_replica(r) for r in range(R)]
    pe = b.potential_ewald(as_array=True)
    b.structure_factor(5)
    for x, y in zip(before, [b.get_replica(r) for r in range(R)]):
        assert all(u.tobytes() == v.tobytes() for u, v in zip(x, y))
    assert pe.tobytes() == b.potential_ewald(as_array=True).tobytes()
    for blk in range(3):
        for b, c in zip(twins, chains):
            b.run_chains(c, 128, T, seed=808 + blk)
        twins[0].structure_factor(5, per_replica=True)
        twins[0].structure_factor(3)
    assert chains[0].tobytes() == chains[1].tobytes()                 # energies and counters
    for r in range(R):                                                # coordinates and S(k)
        for u, v in zip(twins[0].get_replica(r), twins[1].get_replica(r)):
            assert u.tobytes() == v.tobytes()
    assert twins[0].potential_ewald(as_array=True).tobytes() == twins[1].potential_ewald(as_array=True).tobytes()
    for b in twins:
        b.close()
