"""The reference's TIP3P deck (tests/golden/decks: topol.top + tip3p.pdb) through the loaders onto
the device: per-molecule and total energies against the oracle with the deck's own parameters."""
import os

import numpy as np
import pytest

import common
from common import rel

pytestmark = pytest.mark.gpu

DECKS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decks")


def test_tip3p_deck_on_device_matches_oracle():
    from oracle import oracle as orc
    from metropolismontecarlo_amd import io as mio, structs
    from metropolismontecarlo_amd.device import Context
    top = mio.ReadTopFile(os.path.join(DECKS, "topol.top"), substitutions={"SOLNUMBER": 216})
    one = mio.system_from_decks(mio.ReadPDB(os.path.join(DECKS, "tip3p.pdb")), top)
    n_mol = top["molecules"]["SOL"]
    box, com, coords = mio.cubic_lattice_water(n_mol, 0.0331, "tip3p", seed=4)
    # only the water types interact here: restrict the 13-type table to (O1, H)
    a = dict(com=com, coords=coords, first_atom=3 * np.arange(n_mol, dtype=np.int64) + 1,
             last_atom=3 * np.arange(n_mol, dtype=np.int64) + 3,
             atype=np.tile(one["atype"], n_mol), charge=np.tile(one["charge"], n_mol),
             eps=one["eps"][:2, :2].copy(), sig=one["sig"][:2, :2].copy(), box=box)
    rc = 9.0
    assert rc < box / 2
    s = common.oracle_system(a)
    ew = orc.Ewald(5.6 / box, 5, 27, box)
    to = orc.potential_ewald(s, ew, rc, rc)
    with Context() as ctx:
        ctx.upload_system(a["com"], a["first_atom"], a["last_atom"], a["coords"], a["atype"],
                          a["charge"], a["eps"], a["sig"], box)
        ctx.prepare_ewald(5.6 / box, 5, 27, box, structs.factor)
        t = ctx.potential_ewald(rc, rc)
        for key in ("energy", "lj", "real", "recip", "self"):
            assert rel(t[key], to[key]) < 1e-9, key
        for i in (1, n_mol // 2, n_mol):
            e, v = ctx.lj_poly_du(i, rc)
            eo, vo = orc.lj_poly_du(i, s, rc)
            assert rel(e, eo, 1.0) < 1e-9 and rel(v, vo, 1.0) < 1e-9


# ---- the reference's mixture deck: MEA (11 atoms) among TIP3P waters, the full 13-type table ----
RC = 10.0
T_K = 298.15


@pytest.fixture(scope="module")
def mix():
    return common.mea_tip3p_box()


def mix_table():
    """MakeTables(topol.top): all 13 atom types of the deck."""
    from metropolismontecarlo_amd import io as mio
    return mio.MakeTables(mio.ReadTopFile(os.path.join(DECKS, "topol.top"),
                                          substitutions={"SOLNUMBER": 1}))


def mix_ewald_props(box):
    """What Ewald/main.jl:290-303 builds: a dummy EWALD through PrepareEwaldVariables, and the
    simulation properties (temperature, cutoffs, box)."""
    from metropolismontecarlo_amd import structs
    from metropolismontecarlo_amd.api import PrepareEwaldVariables
    from metropolismontecarlo_amd.structs import EWALD, Properties2
    ewald = PrepareEwaldVariables(EWALD(5.6 / box, 5, 27, 1, [[1, 1, 1]] * 3, [0.0, 0.0],
                                        np.zeros(2, complex), np.zeros(2, complex), structs.factor),
                                  box)
    return ewald, Properties2(T_K, 0.0331, 0.0, 0.3166, 0.05, 0.3, 0, 0, [], RC, RC, box)


def _mea(a):
    return [j + 1 for j in range(len(a["com"])) if a["last_atom"][j] - a["first_atom"][j] == 10]


def _rot(rng, dphi):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    t = (rng.random() - 0.5) * 2 * dphi
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def oracle_water_chain(a, n, seed, dr=0.35, dphi=0.25):
    """n rigid water moves (a translation and a rotation about the centre of mass) run by the
    oracle's trial_move, each decided by Metropolis at T_K on the oracle's dU.  Every water that
    follows an MEA in the arrays is proposed first; then waters at random.  Returns the steps
    (mol, com_new, atoms_new, d, overlap, accept) and the final oracle system."""
    from oracle import oracle as orc
    s = common.oracle_system(a)
    ew = orc.Ewald(5.6 / s.box, 5, 27, s.box)
    orc.recip_long(ew, s.coords, s.charge, s.box)
    mea = _mea(a)
    rng = np.random.default_rng(seed)
    waters = [j for j in range(1, len(a["com"]) + 1) if j not in mea]
    seq = [i + 1 for i in mea] + [int(w) for w in rng.choice(waters, n - len(mea))]
    out = []
    for i in seq:
        f, l = int(a["first_atom"][i - 1]), int(a["last_atom"][i - 1])
        c = s.com[i - 1] + (rng.random(3) - 0.5) * 2 * dr
        at = (s.coords[f - 1:l] - s.com[i - 1]) @ _rot(rng, dphi).T + c
        d, ov = orc.trial_move(i, s, ew, RC, RC, c, at)
        du = d[0] + d[1] + d[2]
        acc = (not ov) and (du <= 0 or rng.random() < np.exp(-du / T_K))
        if acc:
            s.com[i - 1] = c
            s.coords[f - 1:l] = at
            ew.sumQExpOld = ew.sumQExpNew.copy()
        else:
            ew.sumQExpNew = ew.sumQExpOld.copy()
        out.append((i, c, at, np.array(d), bool(ov), bool(acc)))
    n_acc = sum(st[5] for st in out)
    assert 0 < n_acc < len(out)
    return out, s


def test_mea_tip3p_totals_context_and_api(mix):
    """Totals of the mixture (Ewald and Wolf) through Context and through api.potential, and the
    per-molecule calls on an MEA and on the waters around it, against the oracle."""
    from oracle import oracle as orc
    from metropolismontecarlo_amd import structs
    from metropolismontecarlo_amd.api import potential, release_sessions
    from metropolismontecarlo_amd.device import Context
    from metropolismontecarlo_amd.structs import Properties
    a = mix
    box = a["box"]
    assert 2 * RC < box and a["eps"].shape == (13, 13)
    s = common.oracle_system(a)
    ew = orc.Ewald(5.6 / box, 5, 27, box)
    to = orc.potential_ewald(s, ew, RC, RC)
    wo = orc.potential_wolf(s, ew, RC, RC, literal_prefactor=False)
    assert to["n_overlap"] == 0
    with Context() as ctx:
        ctx.upload_system(a["com"], a["first_atom"], a["last_atom"], a["coords"], a["atype"],
                          a["charge"], a["eps"], a["sig"], box)
        ctx.prepare_ewald(5.6 / box, 5, 27, box, structs.factor)
        t = ctx.potential_ewald(RC, RC)
        for key in ("energy", "virial", "coulomb", "lj", "real", "recip", "self"):
            assert rel(t[key], to[key]) < 1e-9, (key, t[key], to[key])
        w = ctx.potential_wolf(RC, RC)
        for key in ("energy", "virial", "coulomb", "lj", "real", "self"):
            assert rel(w[key], wo[key], 1.0) < 1e-9, (key, w[key], wo[key])
        for i in sorted(set(_mea(a) + [i + 1 for i in _mea(a)] + [len(a["com"])])):
            p, v = ctx.lj_poly_du(i, RC)
            po, vo = orc.lj_poly_du(i, s, RC)
            assert rel(p, po, 1.0) < 1e-9 and rel(v, vo, abs(po) + 1.0) < 1e-9, (i, p, po)
            e, vq, ov = ctx.ewald_short(i, RC)
            eo, vqo, ovo = orc.ewald_short(i, s, ew, RC)
            assert ov == ovo and rel(e, eo, 1.0) < 1e-9 and rel(vq, vqo, 1.0) < 1e-9, (i, e, eo)
    # the reference's surface: potential(..., "ewald") and the 6-argument (Wolf) form
    try:
        moa = structs.make_moa(a["com"].copy(), a["first_atom"], a["last_atom"])
        soa = structs.make_soa(a["coords"].copy(), a["atype"], a["charge"])
        tab = mix_table()
        assert np.array_equal(tab.eps_ij, a["eps"]) and np.array_equal(tab.sig_ij, a["sig"])
        ewald, props = mix_ewald_props(box)
        tot = potential(moa, soa, Properties(), ewald, tab, props, "ewald")
        assert rel(tot.energy, to["energy"]) < 1e-9 and rel(tot.virial, to["virial"]) < 1e-9
        assert rel(tot.coulomb, to["coulomb"]) < 1e-9
        totw = potential(moa, soa, Properties(), ewald, tab, props)
        assert rel(totw.energy, wo["energy"]) < 1e-9 and rel(totw.coulomb, wo["coulomb"]) < 1e-9
    finally:
        release_sessions()


def test_mea_tip3p_loop_body_with_reference_calls(mix):
    """Loop()'s body (Ewald/main.jl:491-629) written with the reference's own calls -- LJ_poly_ΔU,
    EwaldShort, RecipMove and host-array mutations -- on the mixture, moving waters only, waters
    that follow an MEA in the arrays among them; each step's dU against the oracle's trial_move,
    whose decisions both sides follow.  At the end the running total equals a recompute, and
    moving an MEA stops where the reference stops: RecipMove's `@assert n == 3`."""
    from oracle import oracle as orc
    from metropolismontecarlo_amd import structs
    from metropolismontecarlo_amd.api import (EwaldShort, LJ_poly_ΔU, RecipMove, potential,
                                              release_sessions)
    from metropolismontecarlo_amd.structs import Properties
    a = mix
    box = a["box"]
    chain, s_end = oracle_water_chain(a, 60, seed=21)
    try:
        moa = structs.make_moa(a["com"].copy(), a["first_atom"], a["last_atom"])
        soa = structs.make_soa(a["coords"].copy(), a["atype"], a["charge"])
        tab = mix_table()
        ewald, props = mix_ewald_props(box)
        total = potential(moa, soa, Properties(), ewald, tab, props, "ewald")       # main.jl:408
        running = total.energy
        for i, cn, an, do, ovo, acco in chain:
            f, l = moa.firstAtom[i - 1], moa.lastAtom[i - 1]
            assert l - f == 2
            old_e, old_v = LJ_poly_ΔU(i, moa, soa, tab, RC, box)                  # :491
            e, v, overlap1 = EwaldShort(i, moa, soa, props, ewald, box)           # :501
            old_e += e
            old_v += v
            rm_old, ra_old = moa.COM[i - 1].copy(), soa.coords[f - 1:l].copy()    # :514-515
            moa.COM[i - 1] = cn                                                    # :527
            soa.coords[f - 1:l] = an                                               # :552
            new_e, new_v = LJ_poly_ΔU(i, moa, soa, tab, RC, box)                  # :557
            e, v, overlap2 = EwaldShort(i, moa, soa, props, ewald, box)           # :566
            new_e += e
            new_v += v
            overlap = overlap1 or overlap2
            if not overlap:
                d_rec, ewald = RecipMove(box, ewald, ra_old, an, soa.charge[f - 1:l])   # :581
            else:
                d_rec = 0.0
            delta = new_e - old_e + d_rec                                          # :593
            scale = np.abs(do).max() + 1e4
            assert overlap == ovo, i
            assert abs(delta - (do[0] + do[1] + do[2])) < 1e-9 * scale, (i, delta, do)
            assert abs((new_v - old_v) + d_rec / 3 - do[3]) < 1e-9 * scale, (i, do)
            if acco:
                running += delta
                ewald.sumQExpOld = np.array(ewald.sumQExpNew)                      # :621
            else:
                moa.COM[i - 1] = rm_old                                            # :623
                soa.coords[f - 1:l] = ra_old                                       # :624
                ewald.sumQExpNew = np.array(ewald.sumQExpOld)                      # :628
        assert np.array_equal(moa.COM, s_end.com) and np.array_equal(soa.coords, s_end.coords)
        total2 = potential(moa, soa, Properties(), ewald, tab, props, "ewald")
        assert rel(running, total2.energy) < 1e-9, (running, total2.energy)
        to = orc.potential_ewald(s_end, orc.Ewald(5.6 / box, 5, 27, box), RC, RC)
        assert rel(total2.energy, to["energy"]) < 1e-9
        # an MEA: the energies are there (11 atoms <= 16), the reciprocal move is not (n == 3)
        m = _mea(a)[1]
        f, l = moa.firstAtom[m - 1], moa.lastAtom[m - 1]
        po, _ = orc.lj_poly_du(m, s_end, RC)
        assert rel(LJ_poly_ΔU(m, moa, soa, tab, RC, box)[0], po, 1.0) < 1e-9
        with pytest.raises(AssertionError, match="n == 3"):
            RecipMove(box, ewald, soa.coords[f - 1:l], soa.coords[f - 1:l] + 0.1, soa.charge[f - 1:l])
    finally:
        release_sessions()


def test_mea_tip3p_trial_move_chain(mix):
    """The same water chain through Context.trial_move (the fused generic k_move_eval: the mixture
    is not homogeneous) with accept / reject; the final device state is the oracle's, and a
    trial move of an MEA is refused with the reference's assertion."""
    from oracle import oracle as orc
    from metropolismontecarlo_amd import structs
    from metropolismontecarlo_amd.device import Context
    a = mix
    box = a["box"]
    chain, s_end = oracle_water_chain(a, 80, seed=22)
    with Context() as ctx:
        ctx.upload_system(a["com"], a["first_atom"], a["last_atom"], a["coords"], a["atype"],
                          a["charge"], a["eps"], a["sig"], box)
        ctx.prepare_ewald(5.6 / box, 5, 27, box, structs.factor)
        e0 = ctx.potential_ewald(RC, RC)["energy"]
        running = e0
        for i, cn, an, do, ovo, acco in chain:
            d, ov = ctx.trial_move(i, cn, an, RC, RC)
            assert ov == ovo, i
            assert np.abs(d - do).max() < 1e-9 * (np.abs(do).max() + 1e4), (i, d, do)
            if acco:
                ctx.accept_move()
                running += d[0] + d[1] + d[2]
            else:
                ctx.reject_move()
        com, coords = ctx.download_system()
        assert np.array_equal(com, s_end.com) and np.array_equal(coords, s_end.coords)
        t = ctx.potential_ewald(RC, RC)
        to = orc.potential_ewald(s_end, orc.Ewald(5.6 / box, 5, 27, box), RC, RC)
        assert rel(t["energy"], to["energy"]) < 1e-9 and rel(running, t["energy"]) < 1e-9
        m = _mea(a)[0]
        f, l = a["first_atom"][m - 1], a["last_atom"][m - 1]
        with pytest.raises(AssertionError, match="n == 3"):
            ctx.trial_move(m, com[m - 1], coords[f - 1:l], RC, RC)
