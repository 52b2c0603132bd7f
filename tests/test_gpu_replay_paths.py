"""The oracle replays the two families of device-made chains the other replay tests leave out: the
reference's quaternion route (mmc_batch_set_orientations, mode 1 = the faithful q_to_a, mode 2 =
Allen-Tildesley) and tiny systems (1, 2, 3, 16, 17 and 18 molecules), where the generation window
max(1, n_mol - 1), the n_mol == 1 substitution of k_propose and several steps per launch
(n_mol > MMC_GEN_MAX = 16) branch on the molecule count.

replay() steps one chain on the host: the proposal of every step rebuilt from the exported Philox
draws with the reference's formulas (test_gpu_moves.py), dU from orc.trial_move, Metropolis
(auxillary.jl:106-114) with math.exp and the step's own uniform.  Step for step it is compared
with option "trace_steps" (dU and flags), and at the end with the state the batch holds: centres
of mass, coordinates, orientations and S(k); the totals of that state with orc.potential_ewald.

Tolerances as in test_gpu_batch.py / test_gpu_moves.py: TOL * (|dU| + 1e4) per step, 2e-13 A on
coordinates, 4e-16 per quaternion component and accepted rotation of that molecule (see
_check_final)."""
import functools
import math

import numpy as np
import pytest

import common
from common import rel
from metropolismontecarlo_amd import moves
from metropolismontecarlo_amd import io as mio

pytestmark = pytest.mark.gpu

TOL = 1e-9


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def make_batch(a, R, rcut):
    from metropolismontecarlo_amd import structs
    from metropolismontecarlo_amd.device import Batch
    return Batch(R, a["com"], a["coords"], a["atype"], a["charge"], a["eps"], a["sig"], a["box"],
                 5.6 / a["box"], structs.factor, rcut, rcut)


# ---- systems -------------------------------------------------------------------------------------
def _water(com, quat, db, box, faithful):
    """SPC/E charges and LJ on the sites db, atoms built the reference's way from quat."""
    n_mol = com.shape[0]
    coords = np.concatenate([moves.space_fixed_atoms(com[j], quat[j], db, faithful) for j in range(n_mol)])
    a4 = common.nist_arrays(4, "unwrapped")
    first = 3 * np.arange(n_mol, dtype=np.int64) + 1
    return dict(com=np.array(com, dtype=float), coords=coords, first_atom=first, last_atom=first + 2,
                atype=np.tile([1, 2, 2], n_mol).astype(np.int64),
                charge=np.tile([mio.SPCE_Q_O, mio.SPCE_Q_H, mio.SPCE_Q_H], n_mol), eps=a4["eps"],
                sig=a4["sig"], box=float(box))


@functools.lru_cache(maxsize=None)
def system(name, faithful=True):
    """(arrays, quaternions, body) of a named system.
    "q216": 216 molecules at liquid density (18.7 A), random orientations;
    "window": the image-bound window, see test_image_bound_window_against_the_oracle;
    "tinyN": N molecules in a cluster of 3.1 A spacing in an 18 A box (>= 2 r_cut), random
    orientations -- every molecule has neighbours inside the cutoff."""
    from test_gpu_moves import water_body
    db = water_body(True)
    if name == "q216":
        box, com = mio.InitCubicGrid(216, 0.033101144)
        rng = np.random.default_rng(8)
        quat = np.array([moves.random_quaternion(rng) for _ in range(216)])
    elif name == "window":
        # three molecules per column along z, 8.05 A apart (the gate is r_cut = 8.06 A): the pairs
        # 0-1 and 1-2 of a column sit just inside it, 2-0 is 3.9 A apart through the boundary;
        # columns 10 A apart in x and y do not see each other
        box = 20.0
        com = np.array([(x, y, 1.0 + 8.05 * k) for x in (2.5, 12.5) for y in (2.5, 12.5) for k in range(3)])
        quat = np.tile([1.0, 0.0, 0.0, 0.0], (com.shape[0], 1))   # stretches nothing
    else:
        n = int(name[4:])
        box, rng = 18.0, np.random.default_rng(100 + n)
        nc = int(np.ceil(n ** (1 / 3) - 1e-9))
        sites = np.array([(i, j, k) for i in range(nc) for j in range(nc) for k in range(nc)])[:n]
        com = 5.0 + 3.1 * sites + (rng.random((n, 3)) - 0.5) * 0.4
        quat = np.array([moves.random_quaternion(rng) for _ in range(n)])
    return _water(com, quat, db, box, faithful), quat, db


# ---- the replay ----------------------------------------------------------------------------------
def _image_shift(d, box):
    """What orc.vector1D adds to a coordinate difference d = c2 - c1 (Ewald/boundaries.jl)."""
    return np.where(d >= 0.5 * box, -box, np.where(d <= -0.5 * box, box, 0.0))


def image_crossings(i, com_i, at_i, com, coords, box, gate):
    """Molecules j != i whose centre of mass is within `gate` of com_i (minimum image) while an atom
    pair of (i, j) has a per-atom minimum image that differs from the molecules' -- the pairs on
    which taking the image from the molecule (the kernels' IMG = true variants) is wrong."""
    dc = com - com_i
    sc = _image_shift(dc, box)
    near = ((dc + sc) ** 2).sum(1) < gate * gate
    near[i] = False
    out = []
    for j in np.nonzero(near)[0]:
        da = coords[3 * j:3 * j + 3][None, :, :] - at_i[:, None, :]
        if (_image_shift(da, box) != sc[j]).any():
            out.append(int(j))
    return out


def propose(mode, seed, replica, step, com, atoms, q, db, box, dr, dphi):
    """The move k_propose makes: mode 0 the rigid generator, 1 / 2 the quaternion route with the
    faithful / the Allen-Tildesley q_to_a (the construction of
    test_quaternion_moves_match_the_reference_formulas_draw_by_draw).
    Returns (kind, com_new, atoms_new, q_new, metropolis uniform)."""
    from test_gpu_batch import _rigid_proposal
    from test_gpu_moves import ReferenceOrder, SLOT_METROPOLIS, philox_pair
    if mode == 0:
        kind, c_new, a_new, u = _rigid_proposal(seed, replica, step, com, atoms, box, dr, dphi)
        return kind, c_new, a_new, None, u
    draws = ReferenceOrder(seed, replica, step)
    u = philox_pair(seed, replica, step, SLOT_METROPOLIS)[0]
    if draws.chose_move() < 0.5:                                           # main.jl:519
        draws.start_translation()
        kind, c_new, q_new = 0, moves.random_translate_vector(dr, com, box, draws), q.copy()
    else:
        draws.start_rotation()
        kind, c_new, q_new = 1, com.copy(), moves.random_rotate_quaternion(dphi, q, draws)
    return kind, c_new, moves.space_fixed_atoms(c_new, q_new, db, mode == 1), q_new, u


def replay(orc, a, replica, calls, T, dr, dphi, rcut, quat=None, db=None, probe=False, wolf=False):
    """The chain of global replica index `replica` through the calls [(n_steps, seed, mode), ...]
    one batch makes in a row (mode 0 rigid, 1 / 2 quaternions from `quat`, body `db`): the Philox
    counter continues across calls, the molecule sweep restarts at step 0 of every call.  Returns
    the final com / coords / S(k) / quaternions, the accepted rotations per molecule, the sum of the
    accepted dU, counts, every step's (dU, flags) -- bit 0 accepted, bit 1 overlap, bit 2 rotation
    -- and with `probe` the steps whose old or new state has an image crossing (image_crossings).
    `wolf`: the chain of the reference's `Wolf = true` (main.jl:580-593: deltaRecip = 0), so
    dU = d_lj + d_real and the oracle's S arrays are neither committed nor rolled back; v_acc, the
    sum of the accepted moves' virial changes (main.jl:600-601), then leaves out d_recip / 3."""
    s = common.oracle_system(a)
    box, n_mol = a["box"], a["com"].shape[0]
    ew = orc.Ewald(5.6 / box, 5, 27, box)
    orc.recip_long(ew, s.coords, s.charge, box)
    q = None if quat is None else np.array(quat, dtype=float)
    n_qrot = np.zeros(n_mol, dtype=np.int64)
    e_acc, v_acc, n_acc, n_ovl, n_rot, trace, crossed, rng_off = 0.0, 0.0, 0, 0, 0, [], [], 0
    for n_steps, seed, mode in calls:
        for step in range(n_steps):
            i = step % n_mol
            at_old = s.coords[3 * i:3 * i + 3].copy()
            kind, c_new, a_new, q_new, u = propose(mode, seed, replica, rng_off + step, s.com[i].copy(),
                                                   at_old, None if q is None else q[i], db, box, dr, dphi)
            if probe and (image_crossings(i, s.com[i], at_old, s.com, s.coords, box, rcut)
                          or image_crossings(i, c_new, a_new, s.com, s.coords, box, rcut)):
                crossed.append(len(trace))
            d, ov = orc.trial_move(i + 1, s, ew, rcut, rcut, c_new, a_new)
            delta = d[0] + d[1] if wolf else d[0] + d[1] + d[2]           # main.jl:593
            x = delta / T
            accept = (x < 0.0 or math.exp(-x) > u) and not ov             # main.jl:598
            trace.append((delta, int(accept) | (int(ov) << 1) | (kind << 2)))
            n_ovl += bool(ov)
            n_rot += kind
            if accept:
                e_acc += delta
                v_acc += d[3] - d[2] / 3 if wolf else d[3]                # main.jl:600-601
                n_acc += 1
                s.com[i] = c_new
                s.coords[3 * i:3 * i + 3] = a_new
                if mode:
                    q[i] = q_new
                    n_qrot[i] += kind
                if not wolf:
                    ew.sumQExpOld = ew.sumQExpNew.copy()
            elif not wolf:
                ew.sumQExpNew = ew.sumQExpOld.copy()
        rng_off += n_steps
    return dict(com=s.com, coords=s.coords, S=ew.sumQExpOld, quat=q, n_qrot=n_qrot, e_acc=e_acc, v_acc=v_acc,
                n_acc=n_acc, n_ovl=n_ovl, n_rot=n_rot, trace=trace, crossed=crossed)


@functools.lru_cache(maxsize=None)
def replay_of(name, faithful, replica, calls, T, dr, dphi, rcut, probe=False, wolf=False):
    """replay() of a named system (the same chain is checked under several kernels)."""
    from oracle import oracle as orc
    a, quat, db = system(name, faithful)
    uses_quat = any(m for _, _, m in calls)
    return replay(orc, a, replica, calls, T, dr, dphi, rcut, quat if uses_quat else None, db, probe, wolf)


def _check_trace(o, d_gpu, f_gpu, r, at):
    for step, (delta, flags) in enumerate(o["trace"]):
        assert abs(d_gpu[r, step] - delta) < TOL * (abs(delta) + 1e4), (at, r, step, d_gpu[r, step], delta)
        assert f_gpu[r, step] == flags, (at, r, step, f_gpu[r, step], flags)


def _check_final(orc, a, o, final, r, e0, e1, tot, rcut, at):
    """Final state of local replica r against the replay, and the batch's totals of it (`tot`, a
    record array of potential_ewald) against orc.potential_ewald of the downloaded coordinates.
    Quaternions: 4e-16 per accepted rotation of the molecule.  Each rotation is one product
    rot * old whose rounding (a few ulp of components <= 1) adds to what the old quaternion
    carried, so the difference grows at most linearly along the chain; translations copy the
    quaternion bit for bit."""
    com, coords, S, q = final[r]
    assert np.abs(com - o["com"]).max() < 2e-13 and np.abs(coords - o["coords"]).max() < 2e-13, (at, r)
    assert np.abs(S - o["S"]).max() < 1e-11 * np.abs(o["S"]).max(), (at, r)
    if o["quat"] is not None:
        err = np.abs(q - o["quat"]).max(1)
        assert (err < 4e-16 * np.maximum(o["n_qrot"], 1)).all(), (at, r, err.max(), o["n_qrot"].max())
    assert abs((e1[r] - e0[r]) - o["e_acc"]) < TOL * 1e5, (at, r)
    s = common.oracle_system(dict(a, com=com, coords=coords))
    to = orc.potential_ewald(s, orc.Ewald(5.6 / s.box, 5, 27, s.box), rcut, rcut)
    for key in ("energy", "lj", "real", "recip"):
        assert rel(tot[key][r], to[key]) < TOL, (at, r, key, tot[key][r], to[key])


def run_batch(a, R, rcut, opts, runs, check, quat=None, db=None, faithful=True, trace=0, n_groups=2,
              n_parts=1, replica0=0):
    """One batch through the calls `runs` [(n_steps, seed, mode, T, dr, dphi)]: options `opts`,
    orientations (re)set before each call as its mode says.  Returns e0, e1, the traces of the last
    call, the final state {r: (com, coords, S, quat)} of the replicas in `check` and the totals."""
    with make_batch(a, R, rcut) as b:
        b.set_option("device_moves", 1)
        for k, v in opts.items():
            b.set_option(k, v)
        e0 = b.potential_ewald(as_array=True)["energy"].copy()
        e, mode_now, traces = e0, 0, []
        for n_steps, seed, mode, T, dr, dphi in runs:
            if mode != mode_now:
                if mode:
                    b.set_orientations(quat, db, faithful=mode == 1)
                else:
                    b.set_orientations(None, None)
                mode_now = mode
            if trace:
                b.set_option("trace_steps", n_steps)
            e, st = b.run(n_steps, T, dr, dphi, seed=seed, energies=e, n_groups=n_groups,
                          n_parts=n_parts, n_threads=2, replica0=replica0)
            assert st["moves"] == R * n_steps
            if trace:
                traces.append(b.get_trace(n_steps))
        final = {r: b.get_replica(r) + ((b.get_orientations(r) if mode_now else None),) for r in check}
        tot = b.potential_ewald(as_array=True)
        tot = {k: tot[k].copy() for k in ("energy", "lj", "real", "recip")}
    return e0, e, traces, final, tot, st


# ---- the quaternion route ------------------------------------------------------------------------
Q_RCUT, Q_T, Q_DR, Q_DPHI = 7.0, 298.15, 0.3, 0.3
Q_STEPS = 2 * 216 + 5                      # two sweeps and the start of a third


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("kernel,on_device,parts", [
    pytest.param(2, 0, 3, id="k2-host"), pytest.param(2, 1, 1, id="k2-device"),
    pytest.param(1, 0, 2, id="k1"), pytest.param(0, 0, 0, id="k0"), pytest.param(4, 0, 0, id="k4")])
def test_quaternion_route_stepped_by_the_oracle(mode, kernel, on_device, parts, orc):
    """216 molecules, two sweeps, eight replicas in two groups, a launch per step: every step's dU
    and flags of the replicas at both ends of both groups against the oracle, then the final
    centres of mass, coordinates, quaternions (get_orientations), S(k) and totals.  At r_cut 7 A in
    18.7 A, mode 2 takes the wave kernel's molecule image (0.96 A molecules), mode 1 may not."""
    a, quat, db = system("q216", mode == 1)
    R, seed, replica0, check = 8, 31337, 11, (0, 3, 4, 7)
    opts = dict(kernel=kernel, persistent=0, accept_on_device=on_device)
    e0, e1, traces, final, tot, st = run_batch(a, R, Q_RCUT, opts, [(Q_STEPS, seed, mode, Q_T, Q_DR, Q_DPHI)],
                                               check, quat, db, mode == 1, trace=Q_STEPS, n_parts=parts,
                                               replica0=replica0)
    assert st["device_decisions"] == (R * Q_STEPS if on_device else 0)
    n_rej = n_rot = 0
    for r in check:
        o = replay_of("q216", mode == 1, replica0 + r, ((Q_STEPS, seed, mode),), Q_T, Q_DR, Q_DPHI, Q_RCUT)
        _check_trace(o, *traces[0], r, (mode, kernel))
        _check_final(orc, a, o, final, r, e0, e1, tot, Q_RCUT, (mode, kernel))
        n_rej += Q_STEPS - o["n_acc"]
        n_rot += int(o["n_qrot"].sum())
    assert n_rej > 20 and n_rot > 100


@pytest.mark.parametrize("mode,per_launch", [(1, 8), (1, 16), (2, 8), (2, 16)])
def test_quaternion_route_several_steps_per_launch(mode, per_launch, orc):
    """The kernel decides and one launch takes a replica through 8 or 16 steps (the last launch
    short), one workgroup per launch so that a wave runs three units in turn: no trace on this path,
    so the final state and totals of replicas at the edges of the unit -> wave map against the
    replay."""
    a, quat, db = system("q216", mode == 1)
    R, seed, replica0 = 24, 4242, 3
    check = common.replicas_by_wave_position(R, 2, wave_wgs=1)
    opts = dict(kernel=2, persistent=0, accept_on_device=1, steps_per_launch=per_launch, wave_wgs=1)
    e0, e1, _, final, tot, st = run_batch(a, R, Q_RCUT, opts, [(Q_STEPS, seed, mode, Q_T, Q_DR, Q_DPHI)],
                                          list(check), quat, db, mode == 1, replica0=replica0)
    assert st["device_decisions"] == R * Q_STEPS and st["launches"] == 2 * -(-Q_STEPS // per_launch)
    for r in check:
        o = replay_of("q216", mode == 1, replica0 + r, ((Q_STEPS, seed, mode),), Q_T, Q_DR, Q_DPHI, Q_RCUT)
        _check_final(orc, a, o, final, r, e0, e1, tot, Q_RCUT, (mode, per_launch, check[r]))
        assert 0 < o["n_acc"] < Q_STEPS


# box / 2 = 10 A, gate = r_cut = 8.06 A: the uploaded molecules (0.9645 A) pass the condition of the
# molecule-image kernels (8.06 + 2 * 0.9645 + 1e-6 < 10), while mode 1 reaches 1.09 A along z
W_RCUT, W_T, W_DR, W_DPHI, W_STEPS = 8.06, 1.0e7, 1.0e-3, math.pi, 240


def test_window_fixture_probes_the_window():
    """Host-side precondition of the window tests: the geometry stays where it probes."""
    a, quat, db = system("window", True)
    r_upload = np.linalg.norm(db, axis=1).max()
    reach = max(np.linalg.norm(v) + math.sqrt(2.0) * abs(v[1]) for v in db)
    assert W_RCUT + 2 * r_upload + 1e-6 < a["box"] / 2 < W_RCUT + 2 * reach
    assert np.abs(a["coords"] - np.repeat(a["com"], 3, axis=0) - np.tile(db, (a["com"].shape[0], 1))).max() < 1e-14


def test_image_bound_window_against_the_oracle(orc):
    """Mode 1 from identity quaternions in the window: at temperature 1e7 K and dphi_max = pi the
    orientations wander, molecules deform (quirk Q12) and some atom pair of a gated molecule pair
    crosses box / 2 in z.  The replay must visit such a state (checked on the host: the fixture
    cannot stop probing the window silently); the kernels must then take the per-atom minimum image,
    so every step's dU and flags, the final state and the totals must match the oracle.  Totals also
    at R = 1 (k_potential_one), for the replica whose chain crossed first."""
    a, quat, db = system("window", True)
    R, seed = 48, 5150
    calls = ((W_STEPS, seed, 1),)
    o = {r: replay_of("window", True, r, calls, W_T, W_DR, W_DPHI, W_RCUT, probe=True) for r in range(R)}
    hits = [r for r in range(R) if o[r]["crossed"]]
    assert len(hits) >= 3, hits                       # the precondition
    opts = dict(kernel=2, persistent=0, accept_on_device=0)
    e0, e1, traces, final, tot, _ = run_batch(a, R, W_RCUT, opts, [(W_STEPS, seed, 1, W_T, W_DR, W_DPHI)],
                                              range(R), quat, db, True, trace=W_STEPS)
    for r in range(R):
        _check_trace(o[r], *traces[0], r, ("window", o[r]["crossed"][:3]))
        _check_final(orc, a, o[r], final, r, e0, e1, tot, W_RCUT, "window")
    r1 = hits[0]
    e0, e1, _, final, tot, _ = run_batch(a, 1, W_RCUT, opts, [(W_STEPS, seed, 1, W_T, W_DR, W_DPHI)],
                                         (0,), quat, db, True, n_groups=1, replica0=r1)
    _check_final(orc, a, o[r1], final, 0, e0, e1, tot, W_RCUT, "window R=1")


def test_mode_switch_keeps_the_bound(orc):
    """Mode 1 in the window, then set_orientations(None) and the rigid generator on the deformed
    molecules: the rigid call's every step, its final state and totals against the oracle (the
    bound set for mode 1 must outlive the mode)."""
    a, quat, db = system("window", True)
    R, check = 16, range(16)
    runs = [(W_STEPS, 606, 1, W_T, W_DR, W_DPHI), (W_STEPS, 707, 0, W_T, W_DR, W_DPHI)]
    opts = dict(kernel=2, persistent=0, accept_on_device=0)
    e0, e1, traces, final, tot, _ = run_batch(a, R, W_RCUT, opts, runs, check, quat, db, True, trace=W_STEPS)
    n_cross = 0
    for r in check:
        # one chain: the Philox counter of the rigid call continues from the quaternion call's
        o = replay(orc, a, r, [(W_STEPS, 606, 1), (W_STEPS, 707, 0)], W_T, W_DR, W_DPHI, W_RCUT, quat, db,
                   probe=True)
        n_cross += sum(1 for k in o["crossed"] if k >= W_STEPS)
        _check_trace(dict(o, trace=o["trace"][:W_STEPS]), *traces[0], r, "mode 1")
        _check_trace(dict(o, trace=o["trace"][W_STEPS:]), *traces[1], r, "rigid after mode 1")
        _check_final(orc, a, dict(o, quat=None), final, r, e0, e1, tot, W_RCUT, "mode switch")
    assert n_cross > 0          # the rigid call visits crossings too (host-side precondition)


def test_quaternion_modes_refuse_the_persistent_server():
    """persistent = 1 insists on the move server, which makes rigid proposals only: modes 1 and 2
    must be refused, not run on the rigid generator."""
    from metropolismontecarlo_amd._lib import MMCError
    a, quat, db = system("tiny16", True)
    for mode in (1, 2):
        with make_batch(a, 4, 7.5) as b:
            b.set_option("device_moves", 1)
            b.set_option("persistent", 1)
            b.set_orientations(quat, db, faithful=mode == 1)
            with pytest.raises(MMCError, match="MMC_ERR_UNSUPPORTED"):
                b.run(4, 298.15, 0.3, 0.3, seed=1, energies=np.zeros(4), n_threads=2)


# ---- tiny systems --------------------------------------------------------------------------------
TINY = (1, 2, 3, 16, 17, 18)
T_RCUT, T_T, T_DR, T_DPHI, T_STEPS = 7.5, 298.15, 0.4, 0.5, 60


@pytest.mark.parametrize("n_mol", TINY)
@pytest.mark.parametrize("kernel,on_device,parts", [
    pytest.param(2, 0, 20, id="k2-host-20parts"), pytest.param(2, 1, 1, id="k2-device"),
    pytest.param(1, 0, 20, id="k1-20parts"), pytest.param(0, 0, 20, id="k0-20parts"),
    pytest.param(4, 0, 0, id="k4-16waves")])
def test_tiny_system_rigid_moves_stepped_by_the_oracle(n_mol, kernel, on_device, parts, orc):
    """Rigid device-made moves, a launch per step, every step against the oracle: the generation
    window max(1, n_mol - 1) capped at 16, the n_mol == 1 substitution (the pending accepted record
    is the molecule's state), and more parts than molecules (empty pair parts)."""
    name = f"tiny{n_mol}"
    a, _, _ = system(name, False)
    R, seed, replica0 = 4, 2024 + n_mol, 7
    T = T_T if n_mol > 1 else 0.01      # (one molecule: |dU| of a rotation ~1e-3 K, ~1e-13 K of a translation)
    opts = dict(kernel=kernel, persistent=0, accept_on_device=on_device)
    e0, e1, traces, final, tot, st = run_batch(a, R, T_RCUT, opts, [(T_STEPS, seed, 0, T, T_DR, T_DPHI)],
                                               range(R), trace=T_STEPS, n_parts=parts, replica0=replica0)
    assert st["device_decisions"] == (R * T_STEPS if on_device else 0)
    n_acc = n_rej = 0
    for r in range(R):
        o = replay_of(name, False, replica0 + r, ((T_STEPS, seed, 0),), T, T_DR, T_DPHI, T_RCUT)
        _check_trace(o, *traces[0], r, (n_mol, kernel))
        _check_final(orc, a, o, final, r, e0, e1, tot, T_RCUT, (n_mol, kernel))
        n_acc += o["n_acc"]
        n_rej += T_STEPS - o["n_acc"]
    assert n_acc > 20 and n_rej > 5


@pytest.mark.parametrize("n_mol", [1, 2])
@pytest.mark.parametrize("on_device", [0, 1])
def test_tiny_system_quaternion_mode_stepped_by_the_oracle(n_mol, on_device, orc):
    """Mode 1 at one and two molecules: with one molecule every step re-proposes the molecule of
    the step before, and k_propose must take the pending accepted record's q_new and coordinates."""
    name = f"tiny{n_mol}"
    a, quat, db = system(name, True)
    R, seed, replica0 = 4, 99 + n_mol, 21
    opts = dict(kernel=2, persistent=0, accept_on_device=on_device)
    e0, e1, traces, final, tot, _ = run_batch(a, R, T_RCUT, opts, [(T_STEPS, seed, 1, T_T, T_DR, T_DPHI)],
                                              range(R), quat, db, True, trace=T_STEPS, replica0=replica0)
    n_sub = 0
    for r in range(R):
        o = replay_of(name, True, replica0 + r, ((T_STEPS, seed, 1),), T_T, T_DR, T_DPHI, T_RCUT)
        _check_trace(o, *traces[0], r, (n_mol, on_device))
        _check_final(orc, a, o, final, r, e0, e1, tot, T_RCUT, (n_mol, on_device))
        f = [flags for _, flags in o["trace"]]
        n_sub += sum(1 for k in range(1, T_STEPS) if f[k - 1] & 1 and f[k] & 4)
    assert n_sub > 10        # accepted moves followed by a rotation of the molecule just committed


@pytest.mark.parametrize("n_mol", [17, 18])
def test_tiny_system_several_steps_per_launch(n_mol, orc):
    """17 molecules is the smallest system that takes several steps per launch (n_mol > 16): eight
    steps per launch, a short last launch, one workgroup so that a wave runs two units."""
    name = f"tiny{n_mol}"
    a, _, _ = system(name, False)
    R, seed, n_steps = 8, 555, 61
    opts = dict(kernel=2, persistent=0, accept_on_device=1, steps_per_launch=8, wave_wgs=1)
    e0, e1, _, final, tot, st = run_batch(a, R, T_RCUT, opts, [(n_steps, seed, 0, T_T, T_DR, T_DPHI)], range(R))
    assert st["device_decisions"] == R * n_steps and st["launches"] == 2 * -(-n_steps // 8), st
    for r in range(R):
        o = replay_of(name, False, r, ((n_steps, seed, 0),), T_T, T_DR, T_DPHI, T_RCUT)
        _check_final(orc, a, o, final, r, e0, e1, tot, T_RCUT, (n_mol, "K=8"))
        assert 0 < o["n_acc"] < n_steps


@pytest.mark.parametrize("kernel", [2, 1, 0])
def test_one_molecule_host_proposals(kernel, orc):
    """mmc_batch_eval at n_mol = 1: every step re-proposes the one molecule, so whenever the step
    before was accepted the kernel substitutes that pending record for the molecule's state.
    Three replicas with different accept rules; proposals made from each replica's own state."""
    a, _, _ = system("tiny1", False)
    R, rng = 3, np.random.default_rng(5)
    rules = [lambda n, ov: True, lambda n, ov: False, lambda n, ov: n % 3 != 1]
    s = [common.oracle_system(a) for _ in range(R)]
    ew = [orc.Ewald(5.6 / a["box"], 5, 27, a["box"]) for _ in range(R)]
    for r in range(R):
        orc.recip_long(ew[r], s[r].coords, s[r].charge, a["box"])
    with make_batch(a, R, T_RCUT) as b:
        b.set_option("kernel", kernel)
        b.set_parts(4)
        b.recip_long()
        acc_prev = np.zeros(R, dtype=bool)
        for n in range(24):
            shift = (rng.random(3) - 0.5) * 0.6
            com_new = np.array([s[r].com[0] + shift for r in range(R)])
            at_new = np.array([s[r].coords[:3] + shift for r in range(R)])
            if n % 2:     # a rotation about the centre of mass
                c, sn = math.cos(0.4 + n * 0.1), math.sin(0.4 + n * 0.1)
                Rz = np.array([[c, -sn, 0.0], [sn, c, 0.0], [0.0, 0.0, 1.0]])
                com_new = np.array([s[r].com[0] for r in range(R)])
                at_new = np.array([s[r].com[0] + (s[r].coords[:3] - s[r].com[0]) @ Rz.T for r in range(R)])
            d, ov = b.eval(1, com_new, at_new, acc_prev)
            for r in range(R):
                do, ovo = orc.trial_move(1, s[r], ew[r], T_RCUT, T_RCUT, com_new[r], at_new[r])
                assert ov[r] == ovo, (n, r)
                assert np.abs(d[r] - do).max() < TOL * (np.abs(do).max() + 1e4), (n, r, d[r], do)
                acc = bool(rules[r](n, ovo)) and not ovo
                if acc:
                    s[r].com[0] = com_new[r]
                    s[r].coords[:3] = at_new[r]
                    ew[r].sumQExpOld = ew[r].sumQExpNew.copy()
                else:
                    ew[r].sumQExpNew = ew[r].sumQExpOld.copy()
                acc_prev[r] = acc
        b.settle(acc_prev)
        for r in range(R):
            com, coords, S = b.get_replica(r)
            assert np.array_equal(com, s[r].com) and np.array_equal(coords, s[r].coords), r
            assert np.abs(S - ew[r].sumQExpOld).max() < 1e-11 * np.abs(ew[r].sumQExpOld).max(), r
        tot = b.potential_ewald()
        for r in range(R):
            to = orc.potential_ewald(s[r], orc.Ewald(5.6 / a["box"], 5, 27, a["box"]), T_RCUT, T_RCUT)
            for key in ("energy", "lj", "real", "recip", "self"):
                assert rel(tot[r][key], to[key], 1e-3) < TOL, (r, key)


@pytest.mark.parametrize("n_mol", TINY)
def test_tiny_system_totals(n_mol, orc):
    """potential_ewald of every tiny system: R = 1 (k_potential_one) and R = 3 (k_total_wave, the
    replicas set to different configurations) against the oracle."""
    a, _, _ = system(f"tiny{n_mol}", False)
    b_arr, _, _ = system(f"tiny{n_mol}", True)      # the same molecules, deformed (mode 1 atoms)
    shifted = dict(a, com=a["com"] + 0.37, coords=a["coords"] + 0.37)
    cases = [a, b_arr, shifted]
    want = [orc.potential_ewald(common.oracle_system(c), orc.Ewald(5.6 / c["box"], 5, 27, c["box"]),
                                    T_RCUT, T_RCUT) for c in cases]
    with make_batch(a, 1, T_RCUT) as b:
        t = b.potential_ewald()[0]
        for key in ("energy", "lj", "real", "recip", "self"):
            assert rel(t[key], want[0][key], 1e-3) < TOL, (n_mol, "R=1", key)
    with make_batch(a, 3, T_RCUT) as b:
        for r, c in enumerate(cases):
            b.set_replica(r, c["com"], c["coords"])
        tot = b.potential_ewald()
        for r in range(3):
            for key in ("energy", "lj", "real", "recip", "self"):
                assert rel(tot[r][key], want[r][key], 1e-3) < TOL, (n_mol, r, key)
            assert tot[r]["n_overlap"] == want[r]["n_overlap"]


# ---- SPC/E + TIP3P mixtures: the generic kernel --------------------------------------------------
M_RCUT, M_T, M_DR, M_DPHI = 10.0, 298.15, 0.3, 0.3
M_STEPS = 2 * 100 + 5                      # two sweeps of NIST configuration 1 and the start of a third


@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("order", common.MIX_ORDERS)
def test_mixture_stepped_by_the_oracle(order, parts, orc):
    """A 3-site mixture (common.spce_tip3p_mixture: four atom types, two charge sets, two
    geometries) is not homogeneous, so mmc_batch_run takes kernel 0: moves drawn on the device,
    decided on the host, eight replicas in two groups, 1 and 3 parts per replica.  Every step's dU
    and flags of the replicas at both ends of both groups against the replay, then their final
    state and totals; both species have accepted and rejected moves in every checked chain."""
    a, sp = common.spce_tip3p_mixture(1, order)
    n_mol = a["com"].shape[0]
    R, seed, check = 8, 2718, (0, 3, 4, 7)
    opts = dict(persistent=0, accept_on_device=0)
    e0, e1, traces, final, tot, st = run_batch(a, R, M_RCUT, opts, [(M_STEPS, seed, 0, M_T, M_DR, M_DPHI)],
                                               check, trace=M_STEPS, n_parts=parts)
    assert st["device_decisions"] == 0
    for r in check:
        o = replay(orc, a, r, ((M_STEPS, seed, 0),), M_T, M_DR, M_DPHI, M_RCUT)
        _check_trace(o, *traces[0], r, (order, parts))
        _check_final(orc, a, o, final, r, e0, e1, tot, M_RCUT, (order, parts))
        for species in (0, 1):
            acc = [o["trace"][k][1] & 1 for k in range(M_STEPS) if sp[k % n_mol] == species]
            assert any(acc) and not all(acc), (order, r, species)
