"""A fixed solute in every replica of a batch (include/mmc_hip.h, "A fixed solute") against the oracle on
the N + 1 molecule system (solute_chain_ref.N1: the waters, then the solute with its own atom types):
the terms of scripted trial moves, the totals, the pair energy and the solute-water histograms.

Separate cutoffs (LJ 8.5, real space 9.5 A) so that the two COM gates are two distances; the solute's
reference point sits 0.4 / 0.3 / 0.2 A from three faces of the box, so that the gates, the pairs and
the histograms cross a face, an edge and the corner.  Tolerance of every energy term: solute_ref's
solute_close (1e-9 K scaled by S / 3 beyond three sites, + 1e-13 of the term).  Every test prints
the largest deviation it met before it asserts."""
import numpy as np
import pytest

import common
import solute_chain_ref as scr
import solute_ref as sr
from metropolismontecarlo_amd import _lib
from metropolismontecarlo_amd import structs

pytestmark = pytest.mark.gpu

LJ, QQ, T = 8.5, 9.5, sr.T


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def cfg3():
    return common.nist_arrays(3, "unwrapped")     # 300 SPC/E in 20 A


def make_batch(a, R, lj=LJ, qq=QQ, alpha=5.6):
    from metropolismontecarlo_amd.device import Batch
    b = Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
              alpha / a["box"], structs.factor, lj, qq)
    b.recip_long()
    return b


def solute_of(name, a):
    return {"methane": sr.methane, "cation": sr.cation, "dipole": sr.dipole, "mea": lambda a: sr.mea(),
            "synthetic16": lambda a: sr.synthetic(a, 16, seed=7)}[name](a)


def corner(box):
    return np.array([box - 0.4, 0.3, box - 0.2])


def image_dist(x, c, box):
    d = np.asarray(x, dtype=float) - c
    d = d + common.image_shift(d, box)
    return np.sqrt((d * d).sum(-1))


def scripted_moves(a, sol, mol, lj, qq, seed):
    """[(tag, molecule (1-based), com_new, atoms_new)]: waters placed at (1 -+ 1e-12) of both COM gates
    from the reference point along sr.GATE_DIRS (through a face, inside the box, through the corner),
    a move into an overlap with every sign of charged site, a move out of both cutoffs, one into the
    first shell, and random small moves of the nearest waters."""
    com, coords, box = np.asarray(a["com"]), np.asarray(a["coords"]), float(a["box"])
    n, c, S = com.shape[0], mol[-1], sol.n_sites
    rng = np.random.default_rng(seed)
    order = np.argsort(image_dist(com, c, box))
    cases, nxt = [], [0]

    def rigid(tag, i, target, anchor=None):
        """molecule i moved rigidly so that `anchor` (its COM, or one of its atoms) lands on target"""
        at = coords[3 * i:3 * i + 3]
        d = (com[i] + (target - (com[i] if anchor is None else at[anchor]))) % box - com[i]
        cases.append((tag, i + 1, com[i] + d, at + d))

    def take():
        nxt[0] += 1
        return int(order[(nxt[0] * 7) % n])
    for gi, g in enumerate((lj, qq)):
        for di, d in enumerate(sr.GATE_DIRS):
            for f in (1 - 1e-12, 1 + 1e-12):
                rigid(("gate", gi, di, f < 1), take(), c + g * f * d)
    for sign, slot in ((1, 0), (-1, 1)):          # the water's O on a positive site, an H on a negative one
        sites = [k for k in range(S) if sol.charge[k] * sign > 0]
        if sites:
            rigid(("overlap", sign), take(), mol[sites[0]] + np.array([0.5, 0.0, 0.0]), anchor=slot)
    rigid(("leaves",), int(order[0]), c + (max(lj, qq) + 1.5) * sr.GATE_DIRS[2])
    rigid(("enters",), int(order[-1]), c + 3.4 * sr.GATE_DIRS[1])
    for k in range(6):
        i = int(order[k % n])
        Rm = sr.rotation(rng) if k % 2 else np.eye(3)
        c_new = (com[i] + (rng.random(3) - 0.5) * 0.6) % box
        cases.append((("near", k), i + 1, c_new, c_new + (coords[3 * i:3 * i + 3] - com[i]) @ Rm.T))
    return cases


def check_terms(orc, a, name, R, lj, qq, alpha, seed):
    sol = solute_of(name, a)
    box = float(a["box"])
    mol = sr.placed(sol.offsets, corner(box), sr.rotation(np.random.default_rng(seed)))
    so = sr.SoluteOracle(orc, a, sol, lj, qq, alpha)
    n1 = scr.N1(so, a["com"], a["coords"], mol, box)
    cases = scripted_moves(a, sol, mol, lj, qq, seed)
    worst, bad, n_ov, n_gated = np.zeros(3), [], 0, [0, 0]
    with make_batch(a, R, lj, qq, alpha) as b:
        b.set_solute(sol, mol)
        b.recip_long()
        for k0 in range(0, len(cases), R):
            picks = [cases[(k0 + r) % len(cases)] for r in range(R)]
            d, ov = b.eval([p[1] for p in picks], [p[2] for p in picks], [p[3] for p in picks])
            b.settle(np.zeros(R, dtype=np.int32))
            for r, (tag, i, c_new, a_new) in enumerate(picks):
                do, ovo = n1.trial(i, c_new, a_new)
                n1.rollback()
                n_ov += bool(ovo)
                if bool(ov[r]) != bool(ovo):
                    bad.append((tag, r, "overlap", bool(ov[r]), ovo))
                for t, tn in enumerate(("d_lj", "d_real", "d_recip")):
                    worst[t] = max(worst[t], abs(d[r, t] - do[t]))
                    if not sr.solute_close(d[r, t], do[t], sol.n_sites):
                        bad.append((tag, r, tn, d[r, t], do[t]))
                if tag[0] == "gate":     # the placement is on the side of the gate it claims
                    inside = image_dist(c_new, mol[-1], box) < (lj, qq)[tag[1]]
                    n_gated[int(inside)] += 1
                    if inside != tag[3]:
                        bad.append((tag, "not on its side", image_dist(c_new, mol[-1], box)))
    print(f"terms {name} N={a['com'].shape[0]} R={R}: max |d_lj, d_real, d_recip - oracle| = {worst}, "
          f"{n_ov} overlaps, gate cases outside / inside {n_gated}")
    assert not bad, bad[:8]
    assert n_gated[0] >= 6 and n_gated[1] >= 6
    if np.any(sol.charge != 0):
        assert n_ov >= 1
    return worst


@pytest.mark.parametrize("R", (1, 3, 70))
@pytest.mark.parametrize("N", (1, 2, 65, 257))
def test_terms_of_scripted_moves(orc, cfg3, N, R):
    """d_lj, d_real, d_recip and the overlap flag of mmc_batch_eval with a solute against the oracle's
    trial move on the N + 1 system; the solutes take turns over the shapes."""
    name = ("methane", "cation", "dipole", "synthetic16")[((1, 2, 65, 257).index(N) + (1, 3, 70).index(R)) % 4]
    check_terms(orc, sr.first_molecules(cfg3, N), name, R, LJ, QQ, 5.6, seed=100 * N + R)


@pytest.mark.parametrize("name", ("methane", "cation", "dipole", "synthetic16"))
def test_terms_of_every_solute_at_257(orc, cfg3, name):
    check_terms(orc, sr.first_molecules(cfg3, 257), name, 3, LJ, QQ, 5.6, seed=5)


def test_terms_of_the_decks_mea(orc):
    """The 11-site monoethanolamine of the reference's decks in 65 waters of its TIP3P lattice."""
    check_terms(orc, sr.first_molecules(sr.tip3p_lattice(), 65), "mea", 3, sr.MEA_RCUT, sr.MEA_RCUT, sr.MEA_ALPHA, seed=9)


# ---- totals -------------------------------------------------------------------------------------------
FIELDS = ("energy", "virial", "coulomb", "lj", "real", "recip", "self")


@pytest.fixture(scope="module")
def diversified(cfg3):
    """R = 3 replicas of 257 waters, each 600 device-proposed steps along its own chain."""
    a = sr.first_molecules(cfg3, 257)
    with make_batch(a, 3) as b:
        b.set_option("device_moves", 1)
        b.run(600, T, 0.3, 0.2, seed=77)
        yield a, [b.get_replica(r)[:2] for r in range(3)]


def clear_of_the_water(sol, reps, box, seed):
    """The solute at the corner in the first orientation (seeds seed, seed + 1, ...) that keeps every
    site 1.2 A from every atom of every replica: no overlap, no steric clash whose LJ term would
    swamp the totals it is added to."""
    for k in range(seed, seed + 400):
        mol = sr.placed(sol.offsets, corner(box), sr.rotation(np.random.default_rng(k)))
        ok = True
        for _, coords in reps:
            d = mol[:-1, None, :] - coords[None, :, :]
            d = d + common.image_shift(d, box)
            ok = ok and (d * d).sum(2).min() > 1.2 ** 2
        if ok:
            return mol
    raise AssertionError("no orientation of the solute fits")


def batch_of(a, reps, **kw):
    b = make_batch(a, len(reps), **kw)
    for r, (com, coords) in enumerate(reps):
        b.set_replica(r, com, coords)
    b.recip_long()
    return b


@pytest.mark.parametrize("name", ("methane", "cation", "dipole", "synthetic16"))
def test_totals_are_the_oracles_potential_of_the_n_plus_1_system(orc, diversified, name):
    a, reps = diversified
    sol, box = solute_of(name, a), float(a["box"])
    mol = clear_of_the_water(sol, reps, box, 3)
    so = sr.SoluteOracle(orc, a, sol, LJ, QQ)
    with batch_of(a, reps) as b:
        _, _, du, ovl = b.widom_solute_at(sol, np.tile(mol, (3, 1, 1, 1)), T)
        b.set_solute(sol, mol)
        t1 = b.potential_ewald(as_array=True).copy()
        u_lj, u_real, u_ov = b.solute_energy()
        S_dev = [b.get_replica(r)[2] for r in range(3)]
    worst, bad = {f: 0.0 for f in FIELDS}, []
    for r, (com, coords) in enumerate(reps):
        n1 = scr.N1(so, com, coords, mol, box)
        to = n1.potential()
        for f in FIELDS:
            worst[f] = max(worst[f], abs(t1[f][r] - to[f]) / abs(to[f]) if to[f] else abs(t1[f][r]))
            if not abs(t1[f][r] - to[f]) <= 1e-12 * abs(to[f]):
                bad.append((r, f, t1[f][r], to[f]))
        assert t1["n_overlap"][r] == to["n_overlap"] == 0 and not ovl[r, 0] and not u_ov[r]
        # the pair energy is the insertion's d_lj and d_real, and the oracle's pair sum
        lj_o, real_o, _ = n1.pair_energy()
        for what, x, y in (("u_lj", u_lj[r], lj_o), ("u_real", u_real[r], real_o), ("u_lj", u_lj[r], du[r, 0, 0]),
                           ("u_real", u_real[r], du[r, 0, 1])):
            if not sr.solute_close(x, y, sol.n_sites):
                bad.append((r, what, x, y))
        # S(k) of the N + 1 system
        assert np.abs(S_dev[r] - n1.ew.sumQExpOld).max() < 1e-9, (r, np.abs(S_dev[r] - n1.ew.sumQExpOld).max())
    print(f"totals {name}: largest relative deviation of each field from the oracle {worst}, energy {t1['energy']}")
    assert not bad, bad


@pytest.mark.parametrize("name", ("methane", "cation", "dipole", "synthetic16"))
def test_totals_with_minus_without_a_solute_are_the_insertion_energy(cfg3, name):
    """potential_ewald with a solute minus without one against the sum of mmc_batch_widom_solute_at's
    three terms at the same placement, within solute_close.  On 33 waters: solute_close allows 1e-9 K,
    and a total is a double of its own size -- the self term of 257 SPC/E waters is -7.3e6 K, one ulp of
    which is 9e-10 K, so there the difference of two totals cannot be held to that bound by any
    arithmetic (measured: 2.4e-9 K off for the dipole); of 33 waters it is -9.4e5 K, ulp 1.2e-10 K."""
    a = sr.first_molecules(cfg3, 33)
    sol, box = solute_of(name, a), float(a["box"])
    with make_batch(a, 3) as b:
        b.set_option("device_moves", 1)
        b.set_option("persistent", 0)
        b.run(99, T, 0.3, 0.2, seed=78)
        reps = [b.get_replica(r)[:2] for r in range(3)]
        c = (reps[0][0][5] + 3.1 * sr.GATE_DIRS[2]) % box
        mol = sr.placed(sol.offsets, c, sr.rotation(np.random.default_rng(8)))
        t0 = b.potential_ewald(as_array=True).copy()
        _, _, du, ovl = b.widom_solute_at(sol, np.tile(mol, (3, 1, 1, 1)), T)
        b.set_solute(sol, mol)
        t1 = b.potential_ewald(as_array=True).copy()
    bad = []
    for r in range(3):
        diff, ins = t1["energy"][r] - t0["energy"][r], (du[r, 0, 0] + du[r, 0, 1]) + du[r, 0, 2]
        print(f"totals {name} r={r}: with - without = {diff!r}, widom_solute_at = {ins!r}, self = {t0['self'][r]!r}")
        if ovl[r, 0]:
            assert np.isinf(t1["energy"][r])
        elif not sr.solute_close(diff, ins, sol.n_sites):
            bad.append((r, diff, ins))
    assert not ovl.all() and not bad, bad


def test_an_overlapping_replica_reports_infinity_and_counts(orc, diversified):
    a, reps = diversified
    sol = sr.cation(a)
    mols = [sr.placed(sol.offsets, reps[1][1][3 * 40] + np.array([0.5, 0.0, 0.0]))]    # on the O of water 40 of replica 1
    reps = [(com.copy(), coords.copy()) for com, coords in reps]
    reps[0][0][40, 0] += 2.5                    # ... which in replica 0 is 2.5 A away (a step moves it 0.15 A an axis)
    reps[0][1][120:123, 0] += 2.5
    with batch_of(a, reps) as b:
        b.set_solute(sol, mols[0])
        t = b.potential_ewald(as_array=True)
        u_lj, u_real, ov = b.solute_energy()
    want = [sr.overlaps_water(mols[0][:1], sol.charge, coords, a["charge"][:coords.shape[0]], a["box"]) for _, coords in reps]
    assert want[1] and not all(want)
    for r in range(3):
        assert bool(ov[r]) == want[r]
        if want[r]:
            assert u_real[r] == 0.0 and np.isinf(t["energy"][r]) and t["energy"][r] > 0 and t["n_overlap"][r] == 1
        else:
            assert u_real[r] != 0.0 and np.isfinite(t["energy"][r]) and t["n_overlap"][r] == 0


# ---- S(k): staled by charges only ---------------------------------------------------------------------
def test_an_uncharged_solute_neither_reads_nor_stales_s_of_k(diversified):
    a, reps = diversified
    sol = sr.methane(a)
    with batch_of(a, reps) as b:
        b.set_option("device_moves", 1)
        S0 = [b.get_replica(r)[2].tobytes() for r in range(3)]
        b.set_solute(sol, sr.placed(sol.offsets, corner(a["box"])))
        assert not b.state_info().s_stale
        assert [b.get_replica(r)[2].tobytes() for r in range(3)] == S0
        e = b.potential_ewald(as_array=True)["energy"].copy()
        assert [b.get_replica(r)[2].tobytes() for r in range(3)] == S0      # the fresh sum of the same waters
        b.run(20, T, 0.3, 0.2, seed=5, energies=e)                          # no rebuild was needed
        b.set_solute(None)
        assert not b.state_info().s_stale


def test_a_charged_solute_stales_s_of_k_until_recip_long(diversified):
    a, reps = diversified
    sol = sr.cation(a)
    with batch_of(a, reps) as b:
        b.set_option("device_moves", 1)
        e = b.potential_ewald(as_array=True)["energy"].copy()
        b.set_solute(sol, sr.placed(sol.offsets, corner(a["box"])))
        assert b.state_info().s_stale
        with pytest.raises(_lib.MMCError, match="MMC_ERR_STATE.*stale"):
            b.run(10, T, 0.3, 0.2, seed=5, energies=e)
        with pytest.raises(_lib.MMCError, match="MMC_ERR_STATE.*stale"):
            b.eval(1, np.tile(a["com"][0], (3, 1)), np.tile(a["coords"][:3], (3, 1, 1)))
        b.recip_long()
        assert not b.state_info().s_stale
        b.set_solute(None)                                  # ... and so does taking it away
        assert b.state_info().s_stale
        b.set_solute(sr.methane(a), sr.placed(np.zeros((1, 3)), corner(a["box"])))
        assert b.state_info().s_stale                       # (an uncharged one does not clear the flag)
        b.recip_long()
        assert not b.state_info().s_stale
        got = b.get_solute()
        assert got[0].n_sites == 1 and got[1].tobytes() == sr.placed(np.zeros((1, 3)), corner(a["box"])).tobytes()


# ---- observables --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("methane", "synthetic16"))
@pytest.mark.parametrize("per_replica", (False, True))
def test_rdf_solute_integer_for_integer(diversified, name, per_replica):
    a, reps = diversified
    sol, box = solute_of(name, a), float(a["box"])
    mol = sr.placed(sol.offsets, corner(box), sr.rotation(np.random.default_rng(4)))
    reps = reps * 2                    # six replicas: under wave_wgs = 1 the four waves stride over them
    with batch_of(a, reps) as b:
        b.set_solute(sol, mol)
        for numbins, r_max in ((1, 0.0), (200, 0.0), (1, 6.3), (200, 6.3), (200, box / 2)):
            b.set_option("wave_wgs", 1 if numbins == 200 else 0)     # one workgroup: its waves stride over the replicas
            got = b.rdf_solute(numbins, r_max, per_replica=per_replica)
            want = np.array([scr.rdf_solute_ref(mol, coords, box, numbins, r_max) for _, coords in reps])
            assert got.shape == ((6,) if per_replica else ()) + (1 + sol.n_sites, 3, numbins)
            assert (got == (want if per_replica else want.sum(0))).all(), (numbins, r_max)
            assert want.sum() > 100
        with pytest.raises(_lib.MMCError, match="MMC_ERR_ARG.*r_max"):
            b.rdf_solute(10, box / 2 * (1 + 1e-12))
        b.set_solute(None)
        with pytest.raises(_lib.MMCError, match="MMC_ERR_STATE.*no solute"):
            b.rdf_solute(10)
        with pytest.raises(_lib.MMCError, match="MMC_ERR_STATE.*no solute"):
            b.solute_energy()


def test_solute_energy_is_bitwise_independent_of_the_launch(orc, diversified):
    a, reps = diversified
    sol, box = sr.synthetic(a, 16, seed=7), float(a["box"])
    mol = clear_of_the_water(sol, reps, box, 6)
    so = sr.SoluteOracle(orc, a, sol, LJ, QQ)
    with batch_of(a, reps * 3) as b:   # nine replicas: under wave_wgs = 1 the four waves stride over them
        b.set_solute(sol, mol)
        out = []
        for wgs in (0, 1, 2):
            b.set_option("wave_wgs", wgs)
            out.append(b.solute_energy())
    for o in out[1:]:
        assert all(x.tobytes() == y.tobytes() for x, y in zip(o, out[0]))
    for r, (com, coords) in enumerate(reps):
        lj_o, real_o, ov = scr.N1(so, com, coords, mol, box).pair_energy()
        assert not ov and sr.solute_close(out[0][0][r], lj_o, 16) and sr.solute_close(out[0][1][r], real_o, 16)
        assert out[0][0][r] == out[0][0][r + 3] == out[0][0][r + 6] and out[0][1][r] == out[0][1][r + 6]
