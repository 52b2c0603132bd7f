"""GPU parity, context API (include/mmc_hip.h) vs the CPU oracle, through the C ABI.

Tolerance (BASELINE.json north_star): fp64, 1e-6 relative on totals and per-move dU.  What we
actually hold is far tighter; the asserted bound is TOL = 1e-9 relative (against the magnitude of
the per-molecule energy for differences), leaving room only for summation order and libm-vs-ocml
erfc/sincos/exp differences.  Overlap flags and k-vector tables are bit-exact.
"""
import numpy as np
import pytest

import common
from common import rel

pytestmark = pytest.mark.gpu

TOL = 1e-9
RCUT = 10.0


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_prepare_ewald_bit_exact_kvectors(k, orc):
    a = common.nist_arrays(k)
    ew = orc.Ewald(5.6 / a["box"], 5, 27, a["box"])
    with common.device_context(a) as ctx:
        assert ctx.nkvecs == ew.NKVECS == 337
        kxyz, cfac = ctx.get_kvectors()
        assert np.array_equal(kxyz, ew.kxyz)          # same vectors in the reference's order
        assert np.allclose(cfac, ew.cfac, rtol=1e-14, atol=0)
        so, sn = ctx.get_sumqexp()
        assert not so.any() and not sn.any()           # zeros(ComplexF64, NKVECS) ewalds.jl:98-99


def test_prepare_ewald_assert():
    from metropolismontecarlo_amd.device import Context
    with Context() as ctx:
        with pytest.raises(AssertionError, match="k_sq_max == 27"):
            ctx.prepare_ewald(0.2, 5, 26, 30.0, 1.0)
        # nk < 5 prunes, nk > 5 adds nothing (k^2 < 27)
        n3 = sum(1 for kx in range(4) for ky in range(-3, 4) for kz in range(-3, 4)
                 if 0 < kx * kx + ky * ky + kz * kz < 27)
        assert ctx.prepare_ewald(0.2, 3, 27, 30.0, 1.0) == n3
        assert ctx.prepare_ewald(0.2, 7, 27, 30.0, 1.0) == 337


@pytest.mark.parametrize("k,variant", [(1, "reference"), (1, "unwrapped"), (2, "reference"),
                                       (3, "reference"), (4, "reference"), (4, "unwrapped")])
def test_per_molecule_energies(k, variant, orc):
    a = common.nist_arrays(k, variant)
    s = common.oracle_system(a)
    kappa = 5.6 / s.box
    rng = np.random.default_rng(k)
    mols = sorted(set([1, 2, s.n_mol // 2, s.n_mol] + rng.integers(1, s.n_mol + 1, 12).tolist()))
    with common.device_context(a) as ctx:
        for i in mols:
            p, v = ctx.lj_poly_du(i, RCUT)
            po, vo = orc.lj_poly_du(i, s, RCUT)
            assert rel(p, po) < TOL and rel(v, vo, abs(po)) < TOL, (i, p, po, v, vo)
            e, ov = ctx.ewald_real(i, RCUT)
            eo, ovo = orc.ewald_real(i, s, kappa, RCUT)
            assert ov == ovo and rel(e, eo) < TOL, (i, e, eo)
            es, vs, ov = ctx.ewald_short(i, RCUT)
            eso, vso, _ = orc.ewald_short(i, s, orc.Ewald(kappa, 5, 27, s.box), RCUT)
            assert rel(es, eso) < TOL and rel(vs, vso) < TOL
            e1, ov1 = ctx.ewald_real(i, RCUT, ovr=1.0)  # legacy signature's ovr (ewalds.jl:240)
            e1o, ov1o = orc.ewald_real(i, s, kappa, RCUT, ovr=1.0)
            assert ov1 == ov1o and rel(e1, e1o, 1.0) < TOL
            eb, ovb = ctx.coulomb_real(i, RCUT)
            ebo, ovbo = orc.coulomb_real(i, s, RCUT)
            assert ovb == ovbo and rel(eb, ebo, 1.0) < TOL
        with pytest.raises(AssertionError, match="r_cut == 10.0"):
            ctx.coulomb_real(1, 9.0)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_recip_long_self_and_nist(k, orc):
    a = common.nist_arrays(k)
    s = common.oracle_system(a)
    ew = orc.Ewald(5.6 / s.box, 5, 27, s.box)
    eo = orc.recip_long(ew, s.coords, s.charge, s.box)
    with common.device_context(a) as ctx:
        e = ctx.recip_long()
        assert rel(e, eo) < TOL
        so, sn = ctx.get_sumqexp()
        scale = np.abs(ew.sumQExpNew).max()
        assert np.abs(sn - ew.sumQExpNew).max() < 1e-12 * scale
        assert np.array_equal(so, sn)                    # ewalds.jl:600-601
        self_e = ctx.ewald_self()
        assert rel(self_e, orc.ewald_self(ew, s.charge)) < 1e-13
        # external known answers: NIST E_fourier / E_self, 6 significant digits
        assert rel(e * ew.factor, common.NIST[k]["fourier"]) < 5e-6
        assert rel(self_e, common.NIST[k]["self"]) < 5e-6


@pytest.mark.parametrize("k,variant", [(1, "reference"), (2, "reference"), (3, "unwrapped"),
                                       (4, "reference"), (4, "unwrapped")])
def test_potential_totals(k, variant, orc):
    a = common.nist_arrays(k, variant)
    g = common.golden(k, variant)
    with common.device_context(a) as ctx:
        t = ctx.potential_ewald(RCUT, RCUT)
        for key in ("energy", "virial", "coulomb", "lj", "real", "recip", "self"):
            assert rel(t[key], g["totals_ewald"][key]) < TOL, (key, t[key], g["totals_ewald"][key])
        assert t["n_overlap"] == g["totals_ewald"]["n_overlap"]
        w = ctx.potential_wolf(RCUT, RCUT)
        for key in ("energy", "virial", "coulomb", "lj", "real", "self"):
            assert rel(w[key], g["totals_wolf"][key], 1.0) < TOL, (key, w[key], g["totals_wolf"][key])


@pytest.mark.parametrize("k,variant", [(1, "reference"), (3, "reference"), (4, "reference"),
                                       (4, "unwrapped")])
def test_scripted_moves_call_by_call(k, variant, orc):
    """Loop()'s call sequence (main.jl:491-629) one reference call at a time: LJ_poly_dU,
    EwaldShort, set molecule, LJ_poly_dU, EwaldShort, RecipMove, commit or rollback -- compared
    with the golden chain the oracle produced."""
    a = common.nist_arrays(k, variant)
    g = common.golden(k, variant)
    com, coords = a["com"].copy(), a["coords"].copy()
    with common.device_context(a) as ctx:
        ctx.recip_long()
        for mv in g["moves"]:
            i = mv["mol"]
            cn, an = np.array(mv["com_new"]), np.array(mv["atoms_new"])
            lj0, v0 = ctx.lj_poly_du(i, RCUT)
            q0, qv0, o0 = ctx.ewald_short(i, RCUT)
            r_old = coords[3 * (i - 1):3 * i].copy()
            ctx.set_molecule(i, cn, an)
            lj1, v1 = ctx.lj_poly_du(i, RCUT)
            q1, qv1, o1 = ctx.ewald_short(i, RCUT)
            ov = o0 or o1
            d_rec = 0.0 if ov else ctx.recip_move(r_old, an, a["charge"][3 * (i - 1):3 * i])
            d = np.array([lj1 - lj0, q1 - q0, d_rec, (v1 + qv1) - (v0 + qv0) + d_rec / 3])
            scale = max(abs(lj0), abs(q0), 1.0)
            assert int(ov) == mv["overlap"]
            assert np.abs(d - np.array(mv["d"])).max() < TOL * scale * 10, (d, mv["d"])
            if mv["accept"]:
                ctx.recip_commit()
                com[i - 1], coords[3 * (i - 1):3 * i] = cn, an
            else:
                ctx.set_molecule(i, com[i - 1], coords[3 * (i - 1):3 * i])
                ctx.recip_rollback()
            so, sn = ctx.get_sumqexp()
            assert np.array_equal(so, sn)
            assert rel(np.abs(so).sum(), mv["sum_abs_S_old"]) < 1e-11


@pytest.mark.parametrize("k,variant", [(1, "reference"), (2, "unwrapped"), (4, "reference")])
def test_trial_move_fused(k, variant, orc):
    """mmc_trial_move = the five hot-path calls in one launch; same golden chain."""
    a = common.nist_arrays(k, variant)
    g = common.golden(k, variant)
    with common.device_context(a) as ctx:
        ctx.recip_long()
        for mv in g["moves"]:
            d, ov = ctx.trial_move(mv["mol"], mv["com_new"], mv["atoms_new"], RCUT, RCUT)
            assert int(ov) == mv["overlap"]
            assert np.abs(d - np.array(mv["d"])).max() < 1e-5, (d, mv["d"])
            scale = np.abs(mv["d"]).max() + 1e4
            assert np.abs(d - np.array(mv["d"])).max() < TOL * scale
            if mv["accept"]:
                ctx.accept_move()
            else:
                ctx.reject_move()
            so, sn = ctx.get_sumqexp()
            assert np.array_equal(so, sn)
            assert rel(np.abs(so).sum(), mv["sum_abs_S_old"]) < 1e-11
        # the device state equals the host chain's final state
        com, coords = ctx.download_system()
        s = common.oracle_system(a)
        for mv in g["moves"]:
            if mv["accept"]:
                s.com[mv["mol"] - 1] = mv["com_new"]
                s.coords[3 * (mv["mol"] - 1):3 * mv["mol"]] = mv["atoms_new"]
        assert np.array_equal(com, s.com) and np.array_equal(coords, s.coords)


def test_overlap_sentinel(orc):
    """ewalds.jl:359-360: r^2 < 0.5 with opposite charges -> (0.0, true), partial sum discarded."""
    a = common.nist_arrays(1, "unwrapped")
    # put an H of molecule 7 0.3 A from the O of molecule 3
    a["coords"][3 * 6 + 1] = a["coords"][3 * 2] + np.array([0.3, 0.0, 0.0])
    s = common.oracle_system(a)
    kappa = 5.6 / s.box
    with common.device_context(a) as ctx:
        for i in (3, 7, 11):
            e, ov = ctx.ewald_real(i, RCUT)
            eo, ovo = orc.ewald_real(i, s, kappa, RCUT)
            assert ov == ovo and rel(e, eo, 1.0) < TOL
        assert ctx.ewald_real(3, RCUT) == (0.0, True)
        t = ctx.potential_ewald(RCUT, RCUT)
        ew = orc.Ewald(kappa, 5, 27, s.box)
        to = orc.potential_ewald(s, ew, RCUT, RCUT)
        assert t["n_overlap"] == to["n_overlap"] == 2
        assert rel(t["real"], to["real"]) < TOL and rel(t["energy"], to["energy"]) < TOL


@pytest.mark.parametrize("seed,na", [(1, (3,)), (2, (1, 2, 3, 5)), (3, (11,)), (4, (1,)), (5, (16,)),
                                     (6, (3, 17)), (7, (24,)), (8, (1, 5, 16, 17))])
def test_ragged_random_systems(seed, na, orc):
    """Molecules of different sizes (firstAtom/lastAtom ranges), several atom types, zero-eps
    pairs, n_mol not a multiple of the workgroup size.  Sizes straddle MMC_MAX_ATOMS = 16: the
    totals count every atom of every molecule (k_mol_energy stages a chosen molecule 16 atoms at a
    time), the per-molecule calls take molecules of at most 16 atoms -- next to bigger ones -- and
    refuse bigger ones."""
    from metropolismontecarlo_amd._lib import MMCError
    a = common.random_system(237, 24.0, seed, na_choices=na, n_types=3)
    s = common.oracle_system(a)
    kappa = 5.6 / s.box
    ew = orc.Ewald(kappa, 5, 27, s.box)
    cnt = a["last_atom"] - a["first_atom"] + 1
    small = [i for i in range(1, s.n_mol + 1) if cnt[i - 1] <= 16]
    big = [i for i in range(1, s.n_mol + 1) if cnt[i - 1] > 16]
    assert bool(big) == (max(na) > 16) and bool(small) == (min(na) <= 16)
    # overlaps stay rare: most molecules have an EwaldReal to compare
    real_all = [orc.ewald_real(i, s, kappa, 9.5)[0] for i in range(1, s.n_mol + 1)]
    assert sum(e != 0.0 for e in real_all) > 0.9 * s.n_mol
    sel = sorted(set(i for i in (1, 2, 100, 236, 237) if cnt[i - 1] <= 16) | set(small[:3] + small[-2:]))
    with common.device_context(a) as ctx:
        for i in sel:
            p, v = ctx.lj_poly_du(i, 9.0)
            po, vo = orc.lj_poly_du(i, s, 9.0)
            assert rel(p, po, 1e-3) < TOL and rel(v, vo, abs(po) + 1e-3) < TOL
            e, ov = ctx.ewald_real(i, 9.5)
            eo, ovo = orc.ewald_real(i, s, kappa, 9.5)
            assert ov == ovo and rel(e, eo, 1e-3) < TOL
            e1, ov1 = ctx.ewald_real(i, 9.5, ovr=1.0)
            e1o, ov1o = orc.ewald_real(i, s, kappa, 9.5, ovr=1.0)
            assert ov1 == ov1o and rel(e1, e1o, 1.0) < TOL, (i, e1, e1o)
            es, vs, ovs = ctx.ewald_short(i, 9.5)
            eso, vso, ovso = orc.ewald_short(i, s, ew, 9.5)
            assert ovs == ovso and rel(es, eso, 1.0) < TOL and rel(vs, vso, 1.0) < TOL, (i, es, eso)
            eb, ovb = ctx.coulomb_real(i, RCUT)
            ebo, ovbo = orc.coulomb_real(i, s, RCUT)
            assert ovb == ovbo and rel(eb, ebo, 1.0) < TOL, (i, eb, ebo)
        for i in big[:2] + big[-1:]:
            for call in (lambda: ctx.lj_poly_du(i, 9.0), lambda: ctx.ewald_real(i, 9.5),
                         lambda: ctx.ewald_short(i, 9.5), lambda: ctx.coulomb_real(i, RCUT),
                         lambda: ctx.set_molecule(i, a["com"][i - 1],
                                                  a["coords"][a["first_atom"][i - 1] - 1:a["last_atom"][i - 1]])):
                with pytest.raises(MMCError, match="MMC_ERR_UNSUPPORTED"):
                    call()
        assert rel(ctx.recip_long(), orc.recip_long(ew, s.coords, s.charge, s.box)) < TOL
        assert rel(ctx.ewald_self(), orc.ewald_self(ew, s.charge)) < 1e-13
        t = ctx.potential_ewald(9.0, 9.5)
        to = orc.potential_ewald(s, ew, 9.0, 9.5)
        for key in ("energy", "virial", "lj", "real", "recip", "self"):
            assert rel(t[key], to[key], 1e-3) < TOL, (key, t[key], to[key])
        assert t["n_overlap"] == to["n_overlap"]
        w = ctx.potential_wolf(9.0, 9.5)
        wo = orc.potential_wolf(s, ew, 9.0, 9.5, literal_prefactor=False)
        for key in ("energy", "virial", "lj", "real", "self"):
            assert rel(w[key], wo[key], 1.0) < TOL, (key, w[key], wo[key])
        assert w["n_overlap"] == wo["n_overlap"]


def test_tiny_systems(orc):
    """n_mol = 1 (no neighbours at all) and n_mol = 2."""
    for n in (1, 2):
        a = common.random_system(n, 12.0, 10 + n)
        s = common.oracle_system(a)
        with common.device_context(a) as ctx:
            for i in range(1, n + 1):
                assert rel(ctx.lj_poly_du(i, 5.0)[0], orc.lj_poly_du(i, s, 5.0)[0], 1e-6) < TOL
                e, ov = ctx.ewald_real(i, 5.0)
                eo, ovo = orc.ewald_real(i, s, 5.6 / 12.0, 5.0)
                assert ov == ovo and rel(e, eo, 1e-6) < TOL
            ew = orc.Ewald(5.6 / 12.0, 5, 27, 12.0)
            assert rel(ctx.recip_long(), orc.recip_long(ew, s.coords, s.charge, s.box), 1e-9) < TOL


def test_large_system_chunked_list(orc):
    """n_mol > MMC_LIST_CAP (2048) exercises the chunked neighbour list; compare a few molecules
    with the oracle and the total with the size-independent identity sum_i E_i / 2."""
    from metropolismontecarlo_amd import io as mio, structs
    n_mol = 5000
    box, com, coords = mio.cubic_lattice_water(n_mol, 0.033101144, "spce", seed=11234)
    tab = structs.Tables([mio.SPCE_EPS_O, 0.0], [mio.SPCE_SIGMA_O, 0.0])
    first = 3 * np.arange(n_mol, dtype=np.int64) + 1
    a = dict(com=com, first_atom=first, last_atom=first + 2, coords=coords,
             atype=np.tile([1, 2, 2], n_mol), charge=np.tile([mio.SPCE_Q_O, mio.SPCE_Q_H, mio.SPCE_Q_H], n_mol),
             eps=tab.eps_ij, sig=tab.sig_ij, box=box)
    s = common.oracle_system(a)
    kappa = 5.6 / box
    with common.device_context(a) as ctx:
        sel = [1, 2047, 2048, 2049, 4096, 4999, 5000]
        lj_sum = real_sum = 0.0
        for i in sel:
            p, v = ctx.lj_poly_du(i, RCUT)
            po, vo = orc.lj_poly_du(i, s, RCUT)
            assert rel(p, po) < TOL and rel(v, vo, abs(po)) < TOL
            e, ov = ctx.ewald_real(i, RCUT)
            eo, ovo = orc.ewald_real(i, s, kappa, RCUT)
            assert ov == ovo and rel(e, eo) < TOL
        t = ctx.potential_ewald(RCUT, RCUT)
        ew = orc.Ewald(kappa, 5, 27, box)
        assert rel(t["recip"], orc.recip_long(ew, s.coords, s.charge, box) * ew.factor) < TOL
        assert rel(t["self"], orc.ewald_self(ew, s.charge)) < 1e-12


def test_argument_errors():
    from metropolismontecarlo_amd._lib import MMCError
    from metropolismontecarlo_amd.device import Context
    a = common.nist_arrays(1)
    with Context() as ctx:
        with pytest.raises(MMCError, match="MMC_ERR_STATE"):
            ctx.lj_poly_du(1, RCUT)                       # nothing uploaded
        bad = dict(a)
        bad["last_atom"] = a["last_atom"].copy()
        bad["last_atom"][5] = 10 ** 6
        with pytest.raises(MMCError, match="MMC_ERR_ARG"):
            ctx.upload_system(bad["com"], bad["first_atom"], bad["last_atom"], bad["coords"],
                              bad["atype"], bad["charge"], bad["eps"], bad["sig"], bad["box"])
    with common.device_context(a, ewald=False) as ctx:
        with pytest.raises(MMCError, match="MMC_ERR_ARG"):
            ctx.lj_poly_du(0, RCUT)
        with pytest.raises(MMCError, match="MMC_ERR_ARG"):
            ctx.lj_poly_du(101, RCUT)
        with pytest.raises(MMCError, match="MMC_ERR_STATE"):
            ctx.ewald_real(1, RCUT)                        # EWALD not prepared
        with pytest.raises(MMCError, match="MMC_ERR_STATE"):
            ctx.recip_long()
    with common.device_context(a) as ctx:
        with pytest.raises(AssertionError, match="n == 3"):
            ctx.recip_move(np.zeros((2, 3)), np.zeros((2, 3)), np.zeros(2))
        with pytest.raises(MMCError, match="MMC_ERR_STATE"):
            ctx.accept_move()
