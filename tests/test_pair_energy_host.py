"""CPU tests of the pair-energy restatement (tests/pair_energy_ref.py) and of the host helpers
observables.pair_energy_distribution, pair_energy_profile and energetic_hbonds, on cases whose answer
is known without a computer -- a hydrogen-bonded dimer, a pair at r_OO = sigma, pairs through the
periodic boundary -- and on the NIST SPC/E configurations."""
import math

import numpy as np

import common
import pair_energy_ref as pref
import structure_ref as sref
from metropolismontecarlo_amd import observables as obs, structs

UNIT = 2 ** 20
U_HB = -1132.2                       # Jorgensen's -2.25 kcal/mol in K
BOX = 32.0
QO, QH = -0.8476, 0.4238             # SPC/E
EPS = np.array([[78.1974311, 0.0], [0.0, 0.0]])
SIG = np.array([[3.16555789, 1.58277894], [1.58277894, 0.0]])
ATYPE = np.array([1, 2, 2])
# a water-like molecule with dyadic offsets, hydrogen 1 along +x
OFF = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [-0.25, 0.9375, 0.0]])


def system(site0, flips=None):
    """Molecules with site 0 at `site0` [N, 3] and offsets OFF (mirrored in x where flips): the
    arguments of pref.pair_energy up to `side`."""
    site0 = np.asarray(site0, dtype=float)
    n = site0.shape[0]
    sx = np.ones(n) if flips is None else np.where(np.asarray(flips), -1.0, 1.0)
    off = OFF[None] * np.stack([sx, np.ones(n), np.ones(n)], axis=1)[:, None, :]
    coords = (site0[:, None, :] + off).reshape(-1, 3)
    return coords, np.tile(ATYPE, n), np.tile([QO, QH, QH], n), EPS, SIG, structs.factor


def run(args, numbins=8, r_max=4.0, **kw):
    return pref.pair_energy(*args, BOX, numbins, r_max, **kw)


def test_row_0_is_the_site_0_histogram_of_the_structure_restatement():
    a = common.nist_arrays(1, "unwrapped")
    box, n = a["box"], a["com"].shape[0]
    for numbins, r_max in ((50, 0.0), (1, 0.0), (37, 7.5)):
        o = pref.pair_energy(a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], structs.factor, box, numbins,
                             r_max, 60, -4000.0, 2000.0, U_HB)
        rows = o["rows"]
        want = sref.six_rows(a["coords"], box, numbins, r_max)[0]
        assert rows.dtype == np.int64 and rows.shape == (3, numbins + 2)
        assert np.array_equal(rows[0, :-1], want.astype(np.int64))
        assert rows[0, -1] == n * (n - 1) // 2 - int(want.sum())
        assert rows[1, -1] == 0 and rows[2, -1] == 0 and o["flagged"] == 0
        assert int(o["uhist"].sum()) == int(want.sum()) and int(o["nhb"].sum()) == n
        back = pref.pair_energy(a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], structs.factor, box,
                                numbins, r_max, 60, -4000.0, 2000.0, U_HB, reverse=True)
        for k in ("rows", "uhist", "nhb", "cnt"):
            assert np.array_equal(o[k], back[k]), k


def test_the_linear_hydrogen_bonded_dimer():
    """Donor at (5, 5, 5) with hydrogen 1 pointing along +x at the acceptor's oxygen 2.75 A away: u_C
    from the nine distances written out by hand."""
    r_oo = 2.75
    o = run(system([[5.0, 5.0, 5.0], [5.0 + r_oo, 5.0, 5.0]]))
    # x_ab = (atom a of the donor) - (atom b of the acceptor), both carrying OFF
    h2 = (-0.25, 0.9375)
    d = {"OO": r_oo, "OH1": r_oo + 1.0, "OH2": math.hypot(r_oo - 0.25, h2[1]),
         "H1O": r_oo - 1.0, "H1H1": r_oo, "H1H2": math.hypot(r_oo - 1.25, h2[1]),
         "H2O": math.hypot(r_oo + 0.25, h2[1]), "H2H1": math.hypot(r_oo + 1.25, h2[1]), "H2H2": r_oo}
    terms = [QO * QO / d["OO"], QO * QH / d["OH1"], QO * QH / d["OH2"],
             QH * QO / d["H1O"], QH * QH / d["H1H1"], QH * QH / d["H1H2"],
             QH * QO / d["H2O"], QH * QH / d["H2H1"], QH * QH / d["H2H2"]]
    u_c = structs.factor * math.fsum(terms)
    s6 = (SIG[0, 0] / r_oo) ** 6
    u_lj = 4.0 * EPS[0, 0] * (s6 * s6 - s6)
    b = 6                                                # dr = 0.5: r = 2.75 is bin 6
    assert o["rows"][0].tolist() == [0] * 6 + [1, 0, 0, 0]
    assert abs(int(o["rows"][1, b]) - u_c * UNIT) <= 1 and abs(int(o["rows"][2, b]) - u_lj * UNIT) <= 1
    assert -2000.0 < u_c + u_lj < U_HB                   # a bond by the energetic criterion
    assert o["flagged"] == 0 and o["rows"][1:, :b].sum() == 0 and o["rows"][1:, b + 1:].sum() == 0
    o = run(system([[5.0, 5.0, 5.0], [5.0 + r_oo, 5.0, 5.0]]), n_ebins=6, u_lo=-6000.0, u_hi=0.0, u_hb=U_HB)
    assert o["uhist"].tolist() == [0, 0, 0, 0, 0, 1, 0, 0]         # [-2000, -1000) is slot 5
    assert o["nhb"].tolist() == [0, 2, 0, 0, 0, 0, 0, 0, 0] and o["n_below"] == 1
    # the same pair beyond r_max: counted in the last slot, no energy at all
    o = run(system([[5.0, 5.0, 5.0], [5.0 + r_oo, 5.0, 5.0]]), r_max=2.5, n_ebins=6, u_lo=-6000.0, u_hi=0.0, u_hb=U_HB)
    assert o["rows"][0].tolist() == [0] * 9 + [1] and not o["rows"][1:].any()
    assert not o["uhist"].any() and o["nhb"].tolist() == [2] + [0] * 8


def test_a_pair_at_sigma_has_no_lennard_jones_energy():
    sg = float(SIG[0, 0])
    o = run(system([[0.0, 0.0, 0.0], [sg, 0.0, 0.0]]))   # D = -sigma exactly: s2 = 1, s6 s6 - s6 = 0
    b = int(np.flatnonzero(o["rows"][0])[0])
    assert o["rows"][0, b] == 1 and o["rows"][2, b] == 0 and o["rows"][1, b] != 0


def test_a_pair_across_the_box_face_and_atoms_wrapped_separately():
    inside = run(system([[1.0, 5.0, 5.0], [-2.0, 5.0, 5.0]], flips=[True, False]), n_ebins=60, u_lo=-4000.0,
                 u_hi=2000.0, u_hb=U_HB)
    across = run(system([[1.0, 5.0, 5.0], [30.0, 5.0, 5.0]], flips=[True, False]), n_ebins=60, u_lo=-4000.0,
                 u_hi=2000.0, u_hb=U_HB)
    assert inside["rows"][0, 6] == 1 and inside["rows"][1, 6] != 0
    for k in ("rows", "uhist", "nhb"):
        assert np.array_equal(inside[k], across[k]), k
    # one hydrogen of each molecule stored a box away from its oxygen: e_a is the minimum image
    args = list(system([[1.0, 5.0, 5.0], [30.0, 5.0, 5.0]], flips=[True, False]))
    coords = args[0].copy()
    coords[1, 0] += BOX
    coords[5, 1] -= BOX
    args[0] = coords
    apart = run(args, n_ebins=60, u_lo=-4000.0, u_hi=2000.0, u_hb=U_HB)
    for k in ("rows", "uhist", "nhb"):
        assert np.array_equal(across[k], apart[k]), k


def test_flagged_pairs_enter_row_0_only():
    # molecule 1 on top of molecule 0 (r = 0: not finite), molecule 2 0.5 A from it (LJ beyond 2^20 K)
    o = run(system([[5.0, 5.0, 5.0], [5.0, 5.0, 5.0], [5.5, 5.0, 5.0], [8.0, 5.0, 5.0]]), n_ebins=4, u_lo=-4000.0,
            u_hi=4000.0, u_hb=U_HB)
    assert o["flagged"] == 3 and o["rows"][0].sum() == 6
    assert int(o["uhist"].sum()) == int(o["rows"][0, :-1].sum()) - 3
    assert np.isfinite(o["margins"]["limit"])


def test_the_rows_add_up_to_the_direct_double_sum():
    a = common.nist_arrays(1, "unwrapped")
    box, n = a["box"], a["com"].shape[0]
    o = pref.pair_energy(a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], structs.factor, box, 50, box / 2)
    tc, tl = pref.direct_sum(a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], structs.factor, box, box / 2)
    got = float(o["rows"][1].sum() + o["rows"][2].sum()) / UNIT
    print(f"sum rows 1 + 2 = {got!r} K, direct sum {tc + tl!r} K, difference {got - (tc + tl):.3e}, "
          f"bound {n * 2.0 ** -20:.3e}")
    assert o["flagged"] == 0 and abs(got - (tc + tl)) <= n * 2.0 ** -20
    uc, ulj, cum = obs.pair_energy_profile(o["rows"], n)
    assert abs(cum[-1] * n - (tc + tl)) <= n * 2.0 ** -20 + 1e-9


def test_nist_configuration_2_looks_like_water():
    a = common.nist_arrays(2, "unwrapped")
    n = a["com"].shape[0]
    o = pref.pair_energy(a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], structs.factor, a["box"], 45, 9.0,
                         30, -4000.0, 2000.0, U_HB)
    assert o["rows"][0, :-1].sum() == 7678 and o["flagged"] == 0
    p, mean = obs.energetic_hbonds(o["nhb"])
    print(f"energetic bonds per molecule {mean:.3f}; uhist {o['uhist'].tolist()}")
    assert 3.0 <= mean <= 3.8 and abs(mean - 2.0 * o["n_below"] / n) < 1e-12
    centres, pu = obs.pair_energy_distribution(o["uhist"], n, -4000.0, 2000.0)
    main = int(np.argmax(pu))
    assert abs(centres[main]) <= 100.0                             # the main peak: distant pairs, u ~ 0
    bonded = int(np.argmax(np.where(centres < -2500.0, pu, -1.0)))  # the hydrogen-bond peak
    lo = bonded + int(np.argmin(pu[bonded:main]))
    assert -2500.0 < centres[lo] < -1000.0, centres[lo]
    assert pu[lo] < 0.6 * pu[bonded] and pu[lo] < 0.05 * pu[main]
    assert o["margins"]["hb"] > 0.9 and o["margins"]["edge"] > 2.0 ** -20


def test_the_observables_helpers_on_known_answers():
    uhist = np.array([5, 10, 0, 30, 7], dtype=np.uint64)            # 3 bins over [-300, 300): width 200
    centres, p = obs.pair_energy_distribution(uhist, 10, -300.0, 300.0)
    assert centres.tolist() == [-200.0, 0.0, 200.0] and p.tolist() == [10 / 2000, 0.0, 30 / 2000]
    c2, p2 = obs.pair_energy_distribution(np.stack([uhist, 2 * uhist]), 10, -300.0, 300.0, n_frames=2)
    assert p2.shape == (2, 3) and np.array_equal(p2[1], p) and np.array_equal(p2[0], p / 2)
    rows = np.array([[0, 2, 4, 9], [0, -6 * UNIT, 4 * UNIT, 0], [0, 2 * UNIT, -UNIT, 0]], dtype=np.int64)
    uc, ulj, cum = obs.pair_energy_profile(rows, 4)
    assert np.isnan(uc[0]) and np.isnan(ulj[0])
    assert uc[1:].tolist() == [-3.0, 1.0] and ulj[1:].tolist() == [1.0, -0.25]
    assert cum.tolist() == [0.0, -1.0, -0.25]
    assert obs.pair_energy_profile(np.stack([rows, rows]), 4, n_frames=2)[2][1].tolist() == [0.0, -0.5, -0.125]
    nhb = np.array([1, 0, 2, 3, 4, 0, 0, 0, 0], dtype=np.uint64)
    p, mean = obs.energetic_hbonds(nhb)
    assert p.tolist() == [0.1, 0.0, 0.2, 0.3, 0.4, 0.0, 0.0, 0.0, 0.0] and mean == (4 + 9 + 16) / 10
    p, mean = obs.energetic_hbonds(np.stack([nhb, np.zeros(9, dtype=np.uint64)]))
    assert mean[0] == 2.9 and np.isnan(mean[1])
    for bad in (lambda: obs.energetic_hbonds(np.zeros(8)), lambda: obs.pair_energy_profile(np.zeros((4, 5)), 3),
                lambda: obs.pair_energy_distribution(np.zeros(2), 3, 0.0, 1.0),
                lambda: obs.pair_energy_distribution(np.zeros(5), 3, 1.0, 1.0)):
        try:
            bad()
        except ValueError:
            continue
        raise AssertionError("accepted")
