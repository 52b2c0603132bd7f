"""CPU tests of the fixed solute: the two fields it takes of mmc_state_info's reserved words, the
normalisation of its pair histograms, the restatements the GPU tests compare with, and the
precondition of the GPU tests of the totals -- the oracle's potential of the N + 1 molecule system
minus that of the N waters is the insertion energy solute_ref.SoluteOracle states."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import common
import solute_chain_ref as scr
import solute_ref as sr
from metropolismontecarlo_amd import _lib, checkpoint, observables, structs


def test_solute_fields_sit_in_the_reserved_words_and_the_size_is_unchanged(tmp_path):
    from boundary import HEADER
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mmc_hip.h"\nint main(void){\n'
                    'printf("%zu %zu %zu %zu %zu\\n", sizeof(mmc_state_info), offsetof(mmc_state_info, rigid_only), '
                    'offsetof(mmc_state_info, solute_on), offsetof(mmc_state_info, solute_hash), '
                    'offsetof(mmc_state_info, reserved));\nreturn 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(prog), "-o", str(exe)])
    size, rigid, on, hsh, res = map(int, subprocess.check_output([str(exe)], text=True).split())
    S = _lib.StateInfo
    assert size == C.sizeof(S) == 8 * 42                 # what it was with reserved[10]
    assert (on, hsh, res) == (rigid + 8, rigid + 16, rigid + 24)    # the first two of the ten words
    assert (S.solute_on.offset, S.solute_hash.offset, S.reserved.offset) == (on, hsh, res)
    assert res + 8 * 8 == size
    assert common.header_define("MMC_STATE_VERSION") == "1"


def test_a_header_without_solute_fields_is_a_state_without_a_solute():
    """Files written before there were solutes have neither field; a state without a solute writes
    neither, so such files and their readers stay what they were."""
    from test_checkpoint_host import make_info
    d = make_info()
    assert "solute_on" not in d
    info = checkpoint.info_from_dict(d)
    assert info.solute_on == 0 and info.solute_hash == 0
    assert checkpoint.info_to_dict(info) == d
    with_solute = dict(d, solute_on=1, solute_hash=0xFEDCBA9876543210)
    info = checkpoint.info_from_dict(with_solute)
    assert info.solute_on == 1 and info.solute_hash == 0xFEDCBA9876543210
    assert checkpoint.info_to_dict(info) == with_solute


def test_solute_hash_restatement():
    a = common.nist_arrays(1, "unwrapped")
    sol = sr.dipole(a)
    mol = sr.placed(sol.offsets, [3.0, 4.0, 5.0])
    h = scr.solute_hash(sol, mol)
    assert 0 < h < 2 ** 64 and h == scr.solute_hash(sol, mol.copy())
    assert h != scr.solute_hash(sol, mol + 1e-13)
    other = structs.Solute("d", sol.offsets, sol.charge * (1 + 1e-15), sol.eps, sol.sig)
    assert h != scr.solute_hash(other, mol)
    assert scr.solute_hash(sr.methane(a), np.zeros((2, 3))) != scr.solute_hash(sr.cation(a), np.zeros((2, 3)))
    # FNV-1a of the 8 bytes of n_sites = 1 and 14 doubles of zeros but eps / sig: against a direct loop
    m = sr.methane(a)
    raw = np.int64(1).tobytes() + np.zeros(6).tobytes() + m.charge.tobytes() + m.eps.tobytes() + m.sig.tobytes()
    want = 0xcbf29ce484222325
    for c in raw:
        want = ((want ^ c) * 0x100000001b3) % 2 ** 64
    assert scr.solute_hash(m, np.zeros((2, 3))) == want


def test_normalize_rdf_solute_on_an_ideal_gas_gives_one():
    """Expected counts of an ideal gas of density rho in the shell k dr < r <= (k + 1) dr are rho times
    the shell's exact volume 4 pi ((k + 1)^3 - k^3) dr^3 / 3: g is 1 in every bin to rounding.  And a
    sampled gas (4e5 points, shells of >= 1000 expected points beyond bin 8) is 1 within 5 sigma."""
    n_sites, frames, box, numbins = 750, 64, 30.0, 60
    dr = box / 2 / numbins
    k = np.arange(numbins)
    expected = frames * n_sites / box ** 3 * 4.0 * np.pi * ((k + 1.0) ** 3 - k ** 3) * dr ** 3 / 3.0
    r, g = observables.normalize_rdf_solute(expected, n_sites, dr, frames / box ** 3)
    assert np.allclose(r, (k + 0.5) * dr, rtol=1e-15) and np.abs(g - 1.0).max() < 1e-12
    rng = np.random.default_rng(5)
    pts = rng.random((400000, 3)) * box
    sol = structs.Solute("p", np.zeros((1, 3)), [0.0], np.zeros((1, 3)), np.zeros((1, 3)))
    mol = sr.placed(sol.offsets, [1.0, 29.0, 15.0])                       # near a face and an edge: images count
    hist = scr.rdf_solute_ref(mol, np.repeat(pts, 3, axis=0), box, numbins)
    assert (hist[0] == hist[1]).all() and (hist[0, 0] == hist[0, 2]).all()   # one site: row 1 == row 0
    r, g = observables.normalize_rdf_solute(hist[0, 0], pts.shape[0], dr, 1 / box ** 3)
    sigma = 1.0 / np.sqrt(expected / (frames * n_sites) * pts.shape[0])
    assert (np.abs(g - 1.0)[8:] < 5 * sigma[8:]).all()
    edges, n = observables.coordination_number(hist[0, 0], 1, dr)
    assert np.allclose(edges, (k + 1) * dr) and n[-1] == hist[0, 0].sum()
    assert observables.coordination_number(hist[0, 0], 1, dr, r_shell=3.5) == hist[0, 0][:14].sum()   # 14 dr = 3.5
    assert observables.coordination_number(hist[0, 0], 2, dr, r_shell=0.1) == 0.0


def test_rdf_solute_restatement_counts_what_a_direct_loop_counts():
    a = sr.first_molecules(common.nist_arrays(1, "unwrapped"), 23)
    box = float(a["box"])
    sol = sr.synthetic(a, 3, seed=2)
    mol = sr.placed(sol.offsets, [0.3, 19.8, 10.0])
    for numbins, r_max in ((1, 0.0), (7, 0.0), (7, 6.5), (200, box / 2)):
        dr = r_max / numbins if r_max > 0 else box / 2 / numbins
        want = np.zeros((4, 3, numbins), dtype=np.uint64)
        pts = np.vstack([mol[3:], mol[:3]])
        for row in range(4):
            for j in range(23):
                for slot in range(3):
                    d = pts[row] - a["coords"][3 * j + slot]
                    for q in range(3):
                        if d[q] < -box / 2:
                            d[q] += box
                        elif d[q] > box / 2:
                            d[q] -= box
                    b = int(np.ceil(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) / dr))
                    if 1 <= b <= numbins:
                        want[row, slot, b - 1] += 1
        assert (scr.rdf_solute_ref(mol, a["coords"], box, numbins, r_max) == want).all()


@pytest.mark.parametrize("name", ("methane", "cation", "dipole", "synthetic16"))
def test_oracle_potential_of_n_plus_1_minus_n_is_the_insertion_energy(name):
    """potential(N + 1) - potential(N), field by field, against SoluteOracle.terms of the same
    placement: lj -> d_lj, real -> d_real, recip + self -> d_recip (terms' d_recip carries EwaldSelf of
    the solute).  Tolerance: each total is a sum of ~1e5 terms of magnitude up to the total's own, so a
    difference of two of them carries ~1e-16 sqrt(1e5) ~ 3e-14 of their size; 1e-12 of the totals' size
    plus solute_close's bound on the terms themselves."""
    from oracle import oracle as orc
    a = common.nist_arrays(1, "unwrapped")
    sol = {"methane": sr.methane, "cation": sr.cation, "dipole": sr.dipole,
           "synthetic16": lambda a: sr.synthetic(a, 16, seed=7)}[name](a)
    so = sr.SoluteOracle(orc, a, sol, 9.0, 10.0)
    box = float(a["box"])
    rng = np.random.default_rng(11)
    s0 = common.oracle_system(a)
    t0 = orc.potential_ewald(s0, orc.Ewald(5.6 / box, 5, 27, box, factor=structs.factor), 9.0, 10.0)
    tested = 0
    for _ in range(6):
        mol = sr.placed(sol.offsets, rng.random(3) * box, sr.rotation(rng))
        lj, real, recip, ov = so.terms(a["com"], a["coords"], mol, box)
        if ov or not np.isfinite(lj):
            continue
        t1 = scr.N1(so, a["com"], a["coords"], mol, box).potential()
        for what, got, want, size in (("lj", t1["lj"] - t0["lj"], lj, abs(t0["lj"])),
                                      ("real", t1["real"] - t0["real"], real, abs(t0["real"])),
                                      ("recip", (t1["recip"] - t0["recip"]) + (t1["self"] - t0["self"]), recip,
                                       abs(t0["self"]))):
            assert abs(got - want) <= 1e-12 * size + 1e-9 * max(1.0, sol.n_sites / 3.0) + 1e-13 * abs(want), \
                (name, what, got, want)
        assert t1["n_overlap"] == t0["n_overlap"] == 0
        tested += 1
    assert tested >= 3


def test_host_rng_restatement_is_splitmix64_and_xoshiro256pp():
    """solute_chain_ref.HostRng against the published first outputs of splitmix64 from state 0 and
    against xoshiro256++ stepped by hand from a known state."""
    g = scr.HostRng.__new__(scr.HostRng)
    g.x = 0
    assert [g._splitmix() for _ in range(4)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F,
                                                 0xF88BB8A8724C81EC]
    g.s = [1, 2, 3, 4]
    M = 2 ** 64 - 1
    rotl = lambda x, k: ((x << k) | (x >> (64 - k))) & M                  # noqa: E731
    assert g.next() == (rotl(1 + 4, 23) + 1) & M
    assert g.s == [1 ^ 4 ^ 2, 2 ^ 3 ^ 1, 3 ^ 1 ^ (2 << 17), rotl(4 ^ 2, 45)]
    a, b = scr.HostRng(7, 0), scr.HostRng(7, 1)
    u = [a.uniform() for _ in range(1000)]
    assert all(0.0 <= x < 1.0 for x in u) and 0.45 < np.mean(u) < 0.55 and u[:4] != [b.uniform() for _ in range(4)]
    assert [scr.HostRng(7, 0, 5).uniform()] != u[:1]
    # the proposal: a translation stays rigid and inside the box, a rotation keeps the centre and the shape
    prop = scr.host_proposal(scr.HostRng(3, 2), 20.0, 0.3, 0.25)
    com, atoms = np.array([19.95, 0.02, 10.0]), np.array([[19.95, 0.02, 10.0], [20.7, 0.5, 10.0], [19.2, 0.5, 10.0]])
    kinds = set()
    for step in range(40):
        kind, c_new, a_new, u = prop(step, com, atoms)
        kinds.add(kind)
        assert callable(u) and (0.0 <= c_new).all() and (c_new <= 20.0).all()
        d0, d1 = np.linalg.norm(atoms - com, axis=1), np.linalg.norm(a_new - c_new, axis=1)
        assert np.abs(d0 - d1).max() < 1e-13
        if kind:
            assert (c_new == com).all() and np.abs(a_new - atoms).max() < 1.0 * 0.26
    assert kinds == {0, 1}
