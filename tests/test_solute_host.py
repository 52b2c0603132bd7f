"""CPU tests of the host side of foreign-solute insertion: the Solute built from the reference's
decks, the host mirror of the generator, and -- with the oracle -- a precondition of
tests/test_gpu_solute.py: the MEA insertions it draws split between overlaps and proper energies."""
import os

import numpy as np
import pytest

import common
import solute_ref as sr
from metropolismontecarlo_amd import io as mio
from metropolismontecarlo_amd import observables as obs
from metropolismontecarlo_amd import structs
from metropolismontecarlo_amd.device import philox4x32


def test_mea_from_the_decks():
    top = sr.deck_top()
    sol = sr.mea()
    assert isinstance(sol, structs.Solute) and sol.name == "mea" and sol.n_sites == 11
    m = mio.system_from_decks(mio.ReadPDB(os.path.join(sr.DECKS, "mea.pdb")), top)
    tab = mio.MakeTables(top)
    slots = np.array([1, 2, 2])
    for a in range(11):
        for k in range(3):
            assert sol.eps[a, k] == tab.eps_ij[m["atype"][a] - 1, slots[k] - 1]
            assert sol.sig[a, k] == tab.sig_ij[m["atype"][a] - 1, slots[k] - 1]
    assert np.array_equal(sol.charge, m["charge"])
    # offsets: coordinates minus the mass COM, so their mass-weighted mean vanishes
    com = (m["coords"] * m["mass"][:, None]).sum(0) / m["mass"].sum()
    assert np.abs(sol.offsets - (m["coords"] - com)).max() <= 1e-13
    assert np.abs((sol.offsets * m["mass"][:, None]).sum(0)).max() <= 1e-11
    # the slots by name are the slots by number
    names = [t["name"] for t in top["atomtypes"]]
    by_name = mio.solute_from_decks(os.path.join(sr.DECKS, "mea.pdb"), top, [names[0], names[1], names[1]])
    assert np.array_equal(by_name.eps, sol.eps) and np.array_equal(by_name.sig, sol.sig)
    # some sites carry LJ against the oxygen slot, none against the hydrogens' eps = 0
    assert (sol.eps[:, 0] > 0.001).any() and np.all(sol.eps[:, 1:] == 0.0)


def test_solute_rejects_bad_shapes():
    with pytest.raises(ValueError):
        structs.Solute("none", np.zeros((0, 3)), [], np.zeros((0, 3)), np.zeros((0, 3)))
    with pytest.raises(ValueError):
        structs.Solute("big", np.zeros((17, 3)), np.zeros(17), np.zeros((17, 3)), np.zeros((17, 3)))
    with pytest.raises(ValueError):
        structs.Solute("ragged", np.zeros((2, 3)), np.zeros(3), np.zeros((2, 3)), np.zeros((2, 3)))
    with pytest.raises(ValueError):
        mio.solute_from_decks(os.path.join(sr.DECKS, "mea.pdb"), sr.deck_top(), (1, 2))


def test_the_mirror_with_waters_offsets_is_widoms_bit_for_bit():
    a = common.nist_arrays(1, "unwrapped")
    off = np.asarray(a["coords"][:3]) - np.asarray(a["com"][0])
    seed, draw0, M, box = 0x1234_5678_9abc_def0, (1 << 33) + 3, 12, float(a["box"])
    for r in (0, 5):
        w = obs.widom_molecules(philox4x32, seed, draw0, M, r, box, off)
        s = obs.solute_molecules(philox4x32, seed, draw0, M, r, box, off)
        assert w.shape == (M, 12) and s.shape == (M, 4, 3)
        assert w.tobytes() == s.tobytes()
        # ... and the reference points are the cavity probes
        assert s[:, 3].tobytes() == obs.cavity_points(philox4x32, seed, draw0, M, r, box).tobytes()


def test_the_mirror_keeps_the_solute_rigid():
    sol = sr.mea()
    M, box = 10, 18.69
    mol = obs.solute_molecules(philox4x32, 99, 7, M, 2, box, sol.offsets)
    assert mol.shape == (M, 12, 3)
    c = mol[:, 11]
    assert np.all((c >= 0) & (c < box))
    d_ref = np.linalg.norm(sol.offsets[:, None] - sol.offsets[None, :], axis=2)
    for j in range(M):
        d = np.linalg.norm(mol[j, :11, None] - mol[j, None, :11], axis=2)
        assert np.abs(d - d_ref).max() <= 1e-12
        assert np.abs(np.linalg.norm(mol[j, :11] - c[j], axis=1) - np.linalg.norm(sol.offsets, axis=1)).max() <= 1e-12
    # one site, no offset: the point itself
    one = obs.solute_molecules(philox4x32, 99, 7, M, 2, box, np.zeros((1, 3)))
    assert one[:, 0].tobytes() == one[:, 1].tobytes() == c.tobytes()


def test_ewald_intra_energy_takes_any_number_of_sites():
    sol = sr.mea()
    e = obs.ewald_intra_energy(sol.offsets, sol.charge, 0.3, structs.factor)
    assert np.isfinite(e) and e != 0.0
    assert obs.ewald_intra_energy(np.zeros((1, 3)), [1.0], 0.3, structs.factor) == 0.0


def test_mea_insertions_split_between_overlaps_and_energies():
    """Precondition of test_gpu_solute.py's MEA case: of the insertions it draws (its seed and
    draw0, replicas 0 and 1, 32 each) into the 216-water deck lattice, the share the oracle flags
    as overlapping lies between 1/4 and 3/4 -- both the overlap path and the energies are
    exercised (31 of 64).  (The GPU test inserts into configurations 300 steps along their chains;
    the share is asserted there again.)"""
    from oracle import oracle as orc
    a = sr.tip3p_lattice()
    sol = sr.mea()
    so = sr.SoluteOracle(orc, a, sol, sr.MEA_RCUT, sr.MEA_RCUT, sr.MEA_ALPHA)
    flagged = 0
    for r in (0, 1):
        mol = obs.solute_molecules(philox4x32, sr.MEA_SEED, sr.MEA_DRAW0, 32, r, a["box"], sol.offsets)
        for j in range(32):
            lj, real, recip, ov = so.terms(a["com"], a["coords"], mol[j], a["box"], key="lattice")
            flagged += bool(ov)
            assert np.isfinite(lj) and np.isfinite(recip) and (real == 0.0 if ov else np.isfinite(real))
    assert 16 <= flagged <= 48, flagged
