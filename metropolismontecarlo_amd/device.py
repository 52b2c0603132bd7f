"""Thin object wrappers over the C ABI (include/mmc_hip.h): ``Context`` (one system, the
reference's per-call surface) and ``Batch`` (R replicas, one launch per step).

numpy arrays in, numpy arrays / floats out.  Index conventions are the reference's: molecule
indices, atom ranges and atom types are 1-based.
"""
import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (CHAIN_DTYPE, TOTALS_DTYPE, Move, MoveResult, RunParams, RunStats, Totals, _dp, _i32p, _i64p,
                   check)

PairEnergy = collections.namedtuple("PairEnergy", "rows uhist nhb flagged")  # Batch.pair_energy
Sdf = collections.namedtuple("Sdf", "grid outside noframe")  # Batch.sdf


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _d(a):
    return a.ctypes.data_as(_dp)


def philox4x32(ctr, key):
    """The library's Philox4x32-10 (mmc_philox4x32): four 32-bit words of counter, two of key."""
    c, k, o = (C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), (C.c_uint32 * 4)()
    check(_lib.lib().mmc_philox4x32(c, k, o))
    return list(o)


def _i(a):
    return a.ctypes.data_as(_i64p)


def _selection(sel, n_mol):
    """(int32 array or None, count) of a selection of molecules shared by all replicas: 0-based
    indices, duplicates allowed; None = all n_mol."""
    if sel is None:
        return None, n_mol
    sel_a = np.ascontiguousarray(sel)
    if sel_a.ndim != 1 or not np.issubdtype(sel_a.dtype, np.integer):
        raise ValueError("sel: a 1-d array of integer molecule indices (0-based)")
    if sel_a.size and (sel_a.min() < -2 ** 31 or sel_a.max() >= 2 ** 31):
        raise ValueError("sel: an index does not fit 32 bits")
    sel_a = np.ascontiguousarray(sel_a, dtype=np.int32)
    return sel_a, sel_a.shape[0]


def _output(a, shape, dtype, name="out"):
    """An array the library writes or adds to in place: the caller's `a`, which must be exactly a
    C-contiguous ndarray of that shape and dtype, or a new zero one when `a` is None."""
    if a is None:
        return np.zeros(shape, dtype=dtype)
    if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.shape == shape and a.flags.c_contiguous):
        raise ValueError(f"{name}: a C-contiguous {np.dtype(dtype).name} array of shape {shape}")
    return a


def _outputs(spec, given, where="out", known_only=False):
    """{name: array} for a spec {name: (shape, dtype)}: _output() of every entry, taken from the dict
    `given` (None = none given; `where` names it in a refusal, None for separate arguments).  Keys
    of `given` that are not in the spec are ignored, or refused with known_only."""
    given = {} if given is None else given
    if not isinstance(given, dict):
        raise ValueError(f"{where}: a dict of arrays under names among {sorted(spec)}, not a {type(given).__name__}")
    if known_only and not set(given) <= set(spec):
        raise ValueError(f"{where}: {[k for k in given if k not in spec]} are no outputs of this call; "
                         f"those are {sorted(spec)}")
    return {k: _output(given.get(k), shape, dt, f"{where}[{k!r}]" if where else k)
            for k, (shape, dt) in spec.items()}


def _insertion_outputs(R, M, boltz_sum, n_overlap, mol, du):
    """The outputs of the widom family: the sums boltz_sum and n_overlap (R,), the caller's or new,
    then new arrays: mol (R, M) + `mol` unless that is None, and du (R, M, 3), ovl (R, M) if `du`."""
    spec = {"boltz_sum": ((R,), np.float64), "n_overlap": ((R,), np.int64)}
    if mol is not None:
        spec["mol"] = ((R, M) + mol, np.float64)
    if du:
        spec.update(du=((R, M, 3), np.float64), ovl=((R, M), np.uint8))
    return _outputs(spec, dict(boltz_sum=boltz_sum, n_overlap=n_overlap), where=None)


def _ptr(a):
    """The ctypes pointer to a's data; its element type is a's dtype's."""
    return a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(a.dtype)))


def _ptrs(res, *names):
    """The pointers to res[name] in the order named; None for a name res does not hold."""
    return [_ptr(res[k]) if k in res else None for k in names]


REFERENCE_IDEAL_TERM = 4.60453   # the ideal-gas term Loop() hard-codes in its block line (main.jl:677)


def block_line(chain, block, n_mol, box, ideal_term=REFERENCE_IDEAL_TERM):
    """Loop()'s status line of one block (Ewald/main.jl:667-679) from one row of the chains array
    (mmc_chain_block_line).  ideal_term: the reference's literal 4.60453, or rho * T for
    auxillary.jl:121-123's Pressure(vir, rho, T, vol)."""
    row = np.ascontiguousarray(chain).reshape(1)
    if row.dtype != CHAIN_DTYPE:
        raise ValueError("chain must be a row of the array returned by Batch.new_chains()")
    buf = C.create_string_buffer(512)
    check(_lib.lib().mmc_chain_block_line(row.ctypes.data_as(C.c_void_p), int(block), int(n_mol),
                                          float(box), float(ideal_term), buf, 512))
    return buf.value.decode("utf-8")


def device_count():
    n = C.c_int32()
    check(_lib.lib().mmc_device_count(C.byref(n)))
    return n.value


def exchange_round(n_rungs, energies, temps, rung, seed, round, parity=None, pressure=0.0, volumes=None, replica0=0,
                   attempt=None, accept=None):
    """mmc_exchange_round, the pure host function (no device, no batch): one round of ladder
    exchanges over energies (R,), R = n_ladders * n_rungs.  temps (R,) float64 and rung (R,) int32
    are updated in place; volumes (R,) or None for NVT; parity None = round & 1.  Returns
    (attempt, accept), (n_rungs - 1,) int64 each, accumulated into the caller's when given."""
    e = _f64(energies).ravel()
    R, n_rungs = e.shape[0], int(n_rungs)
    temps = _output(temps, (R,), np.float64, "temps")
    rung = _output(rung, (R,), np.int32, "rung")
    v = None
    if volumes is not None:
        v = _f64(volumes).ravel()
        if v.shape[0] != R:
            raise ValueError(f"one volume per replica: {R} expected, {v.shape[0]} given")
    if n_rungs >= 1 and R % n_rungs:
        raise ValueError(f"{R} replicas are not whole ladders of {n_rungs} rungs")
    res = _outputs({"attempt": ((max(n_rungs - 1, 0),), np.int64), "accept": ((max(n_rungs - 1, 0),), np.int64)},
                   dict(attempt=attempt, accept=accept), where=None)
    par = int(round) & 1 if parity is None else int(parity)
    check(_lib.lib().mmc_exchange_round(R // max(n_rungs, 1), n_rungs, par, int(seed) & (2 ** 64 - 1), int(replica0),
                                        int(round), float(pressure), _d(e), None if v is None else _d(v), _d(temps),
                                        _ptr(rung), *_ptrs(res, "attempt", "accept")))
    return res["attempt"], res["accept"]


class _Handle:
    """Owns one library handle self._h, destroyed by the call self._L.<_destroy>."""
    _destroy = None

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._L, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Context(_Handle):
    """mmc_ctx: one system (one Markov chain) on one GPU."""
    _destroy = "mmc_ctx_destroy"

    def __init__(self, device=0, stream=None):
        self._L = _lib.lib()
        h = C.c_void_p()
        check(self._L.mmc_ctx_create(device, C.c_void_p(stream or 0), C.byref(h)))
        self._h = h
        self.n_mol = self.n_atoms = 0
        self.nkvecs = 0
        self.factor = None

    # -- state ---------------------------------------------------------------------------------
    def upload_system(self, com, first_atom, last_atom, coords, atype, charge, eps, sig, box):
        com, coords, charge = _f64(com).reshape(-1, 3), _f64(coords).reshape(-1, 3), _f64(charge)
        fa, la, at = _i64(first_atom), _i64(last_atom), _i64(atype)
        eps = np.asfortranarray(eps, dtype=np.float64)
        sig = np.asfortranarray(sig, dtype=np.float64)
        nt = eps.shape[0]
        if eps.shape != (nt, nt) or sig.shape != (nt, nt):
            raise ValueError("eps/sig must be square n_types x n_types")
        if not (len(fa) == len(la) == com.shape[0]) or not (len(at) == len(charge) == coords.shape[0]):
            raise ValueError("inconsistent array lengths")
        ef, sf = eps.ravel(order="F").copy(), sig.ravel(order="F").copy()
        check(self._L.mmc_upload_system(self._h, com.shape[0], coords.shape[0], _d(com), _i(fa),
                                        _i(la), _d(coords), _i(at), _d(charge), nt, _d(ef),
                                        _d(sf), float(box)))
        self.n_mol, self.n_atoms = com.shape[0], coords.shape[0]
        self.box = float(box)

    def set_molecule(self, i, com, atoms):
        com, atoms = _f64(com).ravel(), _f64(atoms).ravel()
        check(self._L.mmc_set_molecule(self._h, int(i), _d(com), _d(atoms)))

    def update_system(self, com, coords):
        com, coords = _f64(com).reshape(-1, 3), _f64(coords).reshape(-1, 3)
        if com.shape[0] != self.n_mol or coords.shape[0] != self.n_atoms:
            raise ValueError("update_system: topology changed, create a new Context")
        check(self._L.mmc_update_system(self._h, _d(com), _d(coords)))

    def download_system(self):
        com = np.empty((self.n_mol, 3))
        coords = np.empty((self.n_atoms, 3))
        check(self._L.mmc_download_system(self._h, _d(com), _d(coords)))
        return com, coords

    def synchronize(self):
        check(self._L.mmc_ctx_synchronize(self._h))

    def volume_change(self, new_box, new_kappa):
        """Device part of an NPT volume move (volumeChange.jl:59-80): rescale + rebuild tables."""
        check(self._L.mmc_volume_change(self._h, float(new_box), float(new_kappa)))
        self.box = float(new_box)

    def volume_trial(self, new_box, new_kappa, lj_rcut, qq_rcut):
        """mmc_volume_trial: snapshot on the device, rescale, new tables, total energy at the new
        volume.  Follow with volume_accept() or volume_reject()."""
        t = Totals()
        check(self._L.mmc_volume_trial(self._h, float(new_box), float(new_kappa), float(lj_rcut),
                                       float(qq_rcut), C.byref(t)))
        self._box_before_trial = self.box
        self.box = float(new_box)
        return t.asdict()

    def volume_accept(self):
        check(self._L.mmc_volume_accept(self._h))

    def volume_reject(self):
        check(self._L.mmc_volume_reject(self._h))
        self.box = self._box_before_trial

    # -- a6 ------------------------------------------------------------------------------------
    def prepare_ewald(self, kappa, nk, k_sq_max, box, factor):
        n = C.c_int64()
        check(self._L.mmc_prepare_ewald(self._h, float(kappa), int(nk), int(k_sq_max), float(box),
                                        float(factor), C.byref(n)))
        self.nkvecs = n.value
        self.factor = float(factor)
        return n.value

    def get_kvectors(self):
        kxyz = np.empty((self.nkvecs, 3), dtype=np.int32)
        cfac = np.empty(self.nkvecs)
        check(self._L.mmc_get_kvectors(self._h, _ptr(kxyz), _d(cfac)))
        return kxyz, cfac

    def get_sumqexp(self):
        so = np.empty(self.nkvecs, dtype=np.complex128)
        sn = np.empty(self.nkvecs, dtype=np.complex128)
        check(self._L.mmc_get_sumqexp(self._h, so.view(np.float64).ctypes.data_as(_dp),
                                      sn.view(np.float64).ctypes.data_as(_dp)))
        return so, sn

    def set_sumqexp(self, sum_old=None, sum_new=None):
        so = None if sum_old is None else np.ascontiguousarray(sum_old, dtype=np.complex128)
        sn = None if sum_new is None else np.ascontiguousarray(sum_new, dtype=np.complex128)
        check(self._L.mmc_set_sumqexp(
            self._h, None if so is None else so.view(np.float64).ctypes.data_as(_dp),
            None if sn is None else sn.view(np.float64).ctypes.data_as(_dp)))

    # -- a2..a13 -------------------------------------------------------------------------------
    def lj_poly_du(self, i, r_cut):
        p, v = C.c_double(), C.c_double()
        check(self._L.mmc_lj_poly_du(self._h, int(i), float(r_cut), C.byref(p), C.byref(v)))
        return p.value, v.value

    def ewald_real(self, i, r_cut, ovr=0.5):
        p, o = C.c_double(), C.c_int32()
        check(self._L.mmc_ewald_real(self._h, int(i), float(r_cut), float(ovr), C.byref(p),
                                     C.byref(o)))
        return p.value, bool(o.value)

    def ewald_short(self, i, qq_rcut):
        e, v, o = C.c_double(), C.c_double(), C.c_int32()
        check(self._L.mmc_ewald_short(self._h, int(i), float(qq_rcut), C.byref(e), C.byref(v),
                                      C.byref(o)))
        return e.value, v.value, bool(o.value)

    def coulomb_real(self, i, r_cut):
        p, o = C.c_double(), C.c_int32()
        check(self._L.mmc_coulomb_real(self._h, int(i), float(r_cut), C.byref(p), C.byref(o)))
        return p.value, bool(o.value)

    def recip_long(self):
        e = C.c_double()
        check(self._L.mmc_recip_long(self._h, C.byref(e)))
        return e.value

    def recip_move(self, r_old, r_new, q):
        r_old, r_new, q = _f64(r_old).ravel(), _f64(r_new).ravel(), _f64(q).ravel()
        e = C.c_double()
        check(self._L.mmc_recip_move(self._h, _d(r_old), _d(r_new), _d(q), q.shape[0],
                                     C.byref(e)))
        return e.value

    def recip_commit(self):
        check(self._L.mmc_recip_commit(self._h))

    def recip_rollback(self):
        check(self._L.mmc_recip_rollback(self._h))

    def ewald_self(self):
        e = C.c_double()
        check(self._L.mmc_ewald_self(self._h, C.byref(e)))
        return e.value

    def potential_ewald(self, lj_rcut, qq_rcut):
        t = Totals()
        check(self._L.mmc_potential_ewald(self._h, float(lj_rcut), float(qq_rcut), C.byref(t)))
        return t.asdict()

    def potential_wolf(self, lj_rcut, qq_rcut):
        t = Totals()
        check(self._L.mmc_potential_wolf(self._h, float(lj_rcut), float(qq_rcut), C.byref(t)))
        return t.asdict()

    def trial_move(self, i, com_new, atoms_new, lj_rcut, qq_rcut):
        com_new, atoms_new = _f64(com_new).ravel(), _f64(atoms_new).ravel()
        d = np.zeros(4)
        o = C.c_int32()
        check(self._L.mmc_trial_move(self._h, int(i), _d(com_new), _d(atoms_new), float(lj_rcut),
                                     float(qq_rcut), _d(d), C.byref(o)))
        return d, bool(o.value)

    # ---- single-precision tolerance study (not a reference interface) ----
    def study_f32_total(self, lj_rcut, qq_rcut, mixed=False):
        """{lj, lj_virial, real, recip, n_overlap}: the summed terms of potential() from fp32
        coordinates and arithmetic (mixed: fp64 accumulators)."""
        out = np.zeros(6)
        check(self._L.mmc_study_f32_total(self._h, float(lj_rcut), float(qq_rcut), int(bool(mixed)),
                                          _d(out)))
        return dict(lj=out[0], lj_virial=out[1], real=out[2], recip=out[3], n_overlap=int(out[4]))

    def study_f32_move(self, i, com_new, atoms_new, lj_rcut, qq_rcut, mixed=False):
        com_new, atoms_new = _f64(com_new).ravel(), _f64(atoms_new).ravel()
        d = np.zeros(3)
        o = C.c_int32()
        check(self._L.mmc_study_f32_move(self._h, int(i), _d(com_new), _d(atoms_new),
                                         float(lj_rcut), float(qq_rcut), int(bool(mixed)), _d(d),
                                         C.byref(o)))
        return d, bool(o.value)

    def accept_move(self):
        check(self._L.mmc_accept_move(self._h))

    def stats(self):
        """mmc_ctx_stats: counters of the context's engine (persistent kernel, cache, speculation)."""
        st = (C.c_int64 * 10)()
        check(self._L.mmc_ctx_stats(self._h, st))
        return dict(zip(("cmds", "launches", "retries", "cache_hits", "spec_hits", "spec_miss",
                         "launch_evals", "alive", "look_ahead_hits", "look_ahead_posted"), list(st)))

    def set_option(self, key, value):
        check(self._L.mmc_ctx_set_option(self._h, key.encode(), int(value)))

    def ping(self, n=1000):
        """Average round trip (us) of n empty commands through the running persistent kernel."""
        us = C.c_double()
        check(self._L.mmc_ctx_ping(self._h, int(n), C.byref(us)))
        return us.value

    def reject_move(self):
        check(self._L.mmc_reject_move(self._h))


class Batch(_Handle):
    """mmc_batch: R replicas of one 3-atoms-per-molecule system on one GPU."""
    _destroy = "mmc_batch_destroy"

    def __init__(self, n_replicas, com, coords, atype, charge, eps, sig, box, kappa, factor,
                 lj_rcut, qq_rcut, nk=5, k_sq_max=27, device=0, stream=None):
        self._L = _lib.lib()
        com, coords, charge = _f64(com).reshape(-1, 3), _f64(coords).reshape(-1, 3), _f64(charge)
        at = _i64(atype)
        eps = np.asfortranarray(eps, dtype=np.float64)
        sig = np.asfortranarray(sig, dtype=np.float64)
        nt = eps.shape[0]
        if coords.shape[0] != 3 * com.shape[0]:
            raise AssertionError("n == 3 atoms per molecule (ewalds.jl:740)")
        ef, sf = eps.ravel(order="F").copy(), sig.ravel(order="F").copy()
        h = C.c_void_p()
        check(self._L.mmc_batch_create(device, C.c_void_p(stream or 0), int(n_replicas),
                                       com.shape[0], _d(com), _d(coords), _i(at), _d(charge), nt,
                                       _d(ef), _d(sf), float(box), float(kappa), int(nk),
                                       int(k_sq_max), float(factor), float(lj_rcut),
                                       float(qq_rcut), C.byref(h)))
        self._h = h
        self.R, self.n_mol = int(n_replicas), com.shape[0]
        self.factor = float(factor)
        self.box, self.kappa = float(box), float(kappa)
        self.charge3 = charge[:3].copy()
        # molecule 1 of the configuration the batch was created from, minimum-imaged about its
        # COM (vector1D, ewalds.jl:30-38): the default test molecule of widom()
        d = coords[:3] - com[0]
        self.widom_offsets = d - self.box * np.round(d / self.box)
        self.nkvecs = 337

    def set_replica(self, r, com, coords):
        com, coords = _f64(com).reshape(-1, 3), _f64(coords).reshape(-1, 3)
        check(self._L.mmc_batch_set_replica(self._h, int(r), _d(com), _d(coords)))

    def get_replica(self, r):
        com = np.empty((self.n_mol, 3))
        coords = np.empty((3 * self.n_mol, 3))
        s = np.empty(self.nkvecs, dtype=np.complex128)
        check(self._L.mmc_batch_get_replica(self._h, int(r), _d(com), _d(coords),
                                            s.view(np.float64).ctypes.data_as(_dp)))
        return com, coords, s

    def recip_long(self):
        e = np.empty(self.R)
        check(self._L.mmc_batch_recip_long(self._h, _d(e)))
        return e

    def potential_ewald(self, as_array=False):
        """potential(..., "ewald") of every replica: a list of dicts, or with as_array=True one
        numpy record array (_lib.TOTALS_DTYPE) filled in place by the library."""
        if as_array:
            out = np.zeros(self.R, dtype=TOTALS_DTYPE)
            check(self._L.mmc_batch_potential_ewald(self._h, out.ctypes.data_as(C.c_void_p)))
            return out
        t = (Totals * self.R)()
        check(self._L.mmc_batch_potential_ewald(self._h, t))
        return [x.asdict() for x in t]

    COULOMB_STYLES = ("ewald", "wolf")   # MMC_COULOMB_EWALD, MMC_COULOMB_WOLF

    def set_coulomb_style(self, style):
        """"ewald" (the default) or "wolf": the reference's global `Wolf` (main.jl:75) for the moves
        of eval / settle / run / run_chains.  Wolf moves skip RecipMove and leave S(k) alone; after
        switching back to "ewald" call recip_long() (or potential_ewald()) before the next move."""
        if style not in self.COULOMB_STYLES:
            raise ValueError(f"coulomb style must be one of {self.COULOMB_STYLES}, not {style!r}")
        check(self._L.mmc_batch_set_coulomb_style(self._h, self.COULOMB_STYLES.index(style)))

    @property
    def coulomb_style(self):
        v = C.c_int32()
        check(self._L.mmc_batch_get_coulomb_style(self._h, C.byref(v)))
        return self.COULOMB_STYLES[v.value]

    def potential_wolf(self, as_array=False):
        """potential() of the Wolf overload (energy.jl:864-943) of every replica, in either style:
        a list of dicts, or with as_array=True one numpy record array (_lib.TOTALS_DTYPE)."""
        if as_array:
            out = np.zeros(self.R, dtype=TOTALS_DTYPE)
            check(self._L.mmc_batch_potential_wolf(self._h, out.ctypes.data_as(C.c_void_p)))
            return out
        t = (Totals * self.R)()
        check(self._L.mmc_batch_potential_wolf(self._h, t))
        return [x.asdict() for x in t]

    def eval(self, mol, com_new, atoms_new, accept_prev=None):
        """mol: (R,) 1-based; com_new: (R,3); atoms_new: (R,3,3); accept_prev: (R,) bool."""
        mol = np.broadcast_to(np.asarray(mol, dtype=np.int64), (self.R,))
        com_new = _f64(com_new).reshape(self.R, 3)
        atoms_new = _f64(atoms_new).reshape(self.R, 9)
        acc = np.zeros(self.R, dtype=bool) if accept_prev is None else np.asarray(accept_prev)
        moves = (Move * self.R)()
        for r in range(self.R):
            moves[r].mol = int(mol[r])
            moves[r].accept_prev = int(bool(acc[r]))
            moves[r].com_new[:] = com_new[r].tolist()
            moves[r].atoms_new[:] = atoms_new[r].tolist()
        res = (MoveResult * self.R)()
        check(self._L.mmc_batch_eval(self._h, moves, res))
        out = np.array([[x.d_lj, x.d_real, x.d_recip, x.d_vir] for x in res])
        ov = np.array([bool(x.overlap) for x in res])
        return out, ov

    def set_parts(self, n_parts):
        check(self._L.mmc_batch_set_parts(self._h, int(n_parts)))

    def settle(self, accept):
        a = np.ascontiguousarray(accept, dtype=np.int32)
        check(self._L.mmc_batch_settle(self._h, a.ctypes.data_as(_i32p)))

    def set_option(self, key, value):
        check(self._L.mmc_batch_set_option(self._h, key.encode(), int(value)))

    def cand_stats(self):
        """mmc_batch_cand_stats: what the candidate lists of the move kernel's COM scan did so far."""
        out = (C.c_int64 * 8)()
        check(self._L.mmc_batch_cand_stats(self._h, out))
        keys = ("list_steps", "scan_steps", "refreshes", "bytes", "refresh_launches", "state", "budget", "t_build")
        return dict(zip(keys, (int(v) for v in out)))

    def volume_change(self, new_box, new_kappa):
        check(self._L.mmc_batch_volume_change(self._h, float(new_box), float(new_kappa)))
        self.box, self.kappa = float(new_box), float(new_kappa)

    def volume_trial(self, new_box, new_kappa):
        """mmc_batch_volume_trial (a batch of ONE replica): device-side snapshot, rescale, new
        tables, total energy at the new volume.  Follow with volume_accept() or volume_reject().
        self.box and self.kappa are the trial's until a reject puts the old ones back."""
        t = Totals()
        check(self._L.mmc_batch_volume_trial(self._h, float(new_box), float(new_kappa), C.byref(t)))
        self._before_trial = (self.box, self.kappa)
        self.box, self.kappa = float(new_box), float(new_kappa)
        return t.asdict()

    def volume_accept(self):
        check(self._L.mmc_batch_volume_accept(self._h))

    def volume_reject(self):
        check(self._L.mmc_batch_volume_reject(self._h))
        self.box, self.kappa = self._before_trial

    def run_npt(self, n_sweeps, temperature, pressure, vmax, dr_max, dphi_max, seed, energy,
                moves_per_sweep=0, alpha=5.6, n_parts=0, n_threads=1, replica0=0):
        """mmc_batch_run_npt: n_sweeps x { moves_per_sweep trial moves (0 = one per molecule), one
        volume move (Ewald/volumeChange.jl:59-147) }.  Returns (energy, run stats, npt stats)."""
        from ._lib import NptParams, NptStats
        p = RunParams(float(temperature), float(dr_max), float(dphi_max), int(seed), 0, 1,
                      int(n_parts), 0, int(n_threads), 0, 0, int(replica0))
        q = NptParams(float(pressure), float(vmax), float(alpha), int(n_sweeps), int(moves_per_sweep))
        st, ns = RunStats(), NptStats()
        e = np.array([float(energy)])
        try:
            check(self._L.mmc_batch_run_npt(self._h, C.byref(p), C.byref(q), _d(e), C.byref(st), C.byref(ns)))
        finally:
            # every accepted volume move set kappa = alpha / L_new (also before an error part-way)
            box = float(self.get_boxes()[0])
            if box != self.box:
                self.box, self.kappa = box, float(alpha) / box
        return float(e[0]), st.asdict(), ns.asdict()

    def set_boxes(self, boxes, alpha=5.6):
        """mmc_batch_set_boxes: per-replica mode, replica r in box boxes[r] with kappa = alpha /
        boxes[r].  The coordinates are not rescaled; call recip_long() afterwards."""
        bx = _f64(boxes).ravel()
        if bx.shape[0] != self.R:
            raise ValueError(f"one box per replica: {self.R} expected, {bx.shape[0]} given")
        check(self._L.mmc_batch_set_boxes(self._h, _d(bx), float(alpha)))

    def get_boxes(self):
        out = np.empty(self.R)
        check(self._L.mmc_batch_get_boxes(self._h, _d(out)))
        return out

    def volume_trial_replicas(self, new_boxes):
        """mmc_batch_volume_trial_replicas: new_boxes[r] == 0 leaves replica r in place.  Returns
        the totals of every replica at its trial box (numpy record array, _lib.TOTALS_DTYPE).
        Follow with volume_settle()."""
        nb = _f64(new_boxes).ravel()
        if nb.shape[0] != self.R:
            raise ValueError(f"one box per replica: {self.R} expected, {nb.shape[0]} given")
        out = np.zeros(self.R, dtype=TOTALS_DTYPE)
        check(self._L.mmc_batch_volume_trial_replicas(self._h, _d(nb),
                                                      out.ctypes.data_as(C.POINTER(Totals))))
        return out

    def volume_settle(self, accept):
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(accept), (self.R,)), dtype=np.int32)
        check(self._L.mmc_batch_volume_settle(self._h, a.ctypes.data_as(_i32p)))

    def run_npt_replicas(self, n_sweeps, temperature, pressure, vmax, dr_max, dphi_max, seed,
                         energies, moves_per_sweep=0, alpha=5.6, n_parts=0, n_threads=1,
                         pressures=None, replica0=0):
        """mmc_batch_run_npt_replicas: mmc_batch_run_npt's chain for every replica of a batch with
        per-replica boxes; `pressures` (R values) overrides `pressure` per replica.  Returns
        (energies, run stats, [per-replica npt stats])."""
        from ._lib import NptParams, NptStats
        p = RunParams(float(temperature), float(dr_max), float(dphi_max), int(seed), 0, 1,
                      int(n_parts), 0, int(n_threads), 0, 0, int(replica0))
        q = NptParams(float(pressure), float(vmax), float(alpha), int(n_sweeps), int(moves_per_sweep))
        e = _f64(energies).ravel().copy()
        if e.shape[0] != self.R:
            raise ValueError(f"one energy per replica: {self.R} expected, {e.shape[0]} given")
        pr = None
        if pressures is not None:
            pr = _f64(pressures).ravel()
            if pr.shape[0] != self.R:
                raise ValueError(f"one pressure per replica: {self.R} expected, {pr.shape[0]} given")
        st, ns = RunStats(), (NptStats * self.R)()
        check(self._L.mmc_batch_run_npt_replicas(self._h, C.byref(p), C.byref(q),
                                                 None if pr is None else _d(pr), _d(e), C.byref(st), ns))
        return e, st.asdict(), [x.asdict() for x in ns]

    def qq_table(self, r2, replica=None):
        """The fast kernel's erfc(kappa r)/r at r^2: mmc_batch_qq_table, or with `replica`
        mmc_batch_qq_table_replica (that replica's own table and kappa under per-replica boxes)."""
        r2 = _f64(r2).ravel()
        out = np.empty_like(r2)
        if replica is None:
            check(self._L.mmc_batch_qq_table(self._h, _d(r2), r2.shape[0], _d(out)))
        else:
            check(self._L.mmc_batch_qq_table_replica(self._h, int(replica), _d(r2), r2.shape[0],
                                                     _d(out)))
        return out

    def run(self, n_steps, temperature, dr_max, dphi_max, seed, energies=None, n_groups=2,
            n_parts=0, time_kernels=False, n_threads=1, n_streams=0, replica0=0):
        """mmc_batch_run.  Chain r draws from the stream (seed, replica0 + r): `replica0` is the
        global index of this batch's first chain when an ensemble is spread over several GPUs."""
        p = RunParams(float(temperature), float(dr_max), float(dphi_max), int(seed), int(n_steps),
                      int(n_groups), int(n_parts), int(time_kernels), int(n_threads),
                      int(n_streams), 0, int(replica0))
        st = RunStats()
        e = np.zeros(self.R) if energies is None else _f64(energies).copy()
        check(self._L.mmc_batch_run(self._h, C.byref(p), _d(e), C.byref(st)))
        return e, st.asdict()

    def set_temperatures(self, temps):
        """mmc_batch_set_temperatures: replica r's moves (run, run_chains, run_npt_replicas and its
        volume criterion) are decided at temps[r]; the `temperature` of those calls is then ignored.
        None switches the array off.  widom*, deletion and volume_perturb keep their own argument."""
        if temps is None:
            check(self._L.mmc_batch_set_temperatures(self._h, None))
            return
        t = _f64(temps).ravel()
        if t.shape[0] != self.R:
            raise ValueError(f"one temperature per replica: {self.R} expected, {t.shape[0]} given")
        check(self._L.mmc_batch_set_temperatures(self._h, _d(t)))

    def temperatures(self):
        """mmc_batch_get_temperatures: the array as exchanges have left it; zeros when off."""
        out = np.empty(self.R)
        check(self._L.mmc_batch_get_temperatures(self._h, _d(out)))
        return out

    def _ladder_arrays(self, n_rungs, energies, rung, attempt, accept):
        """The in/out arrays of an exchange: energies (R,) float64 read, rung (R,) int32 updated in
        place, the counters (n_rungs - 1,) int64 the caller's or new."""
        e = _f64(energies).ravel()
        if e.shape[0] != self.R:
            raise ValueError(f"one energy per replica: {self.R} expected, {e.shape[0]} given")
        rung = _output(rung, (self.R,), np.int32, "rung")
        res = _outputs({"attempt": ((max(int(n_rungs) - 1, 0),), np.int64), "accept": ((max(int(n_rungs) - 1, 0),), np.int64)},
                       dict(attempt=attempt, accept=accept), where=None)
        return e, rung, res

    def exchange(self, n_rungs, energies, rung, seed, round, parity=None, pressure=0.0, replica0=0, attempt=None,
                 accept=None):
        """mmc_batch_exchange: one round of ladder exchanges (exchange_round) on the batch's own
        temperatures; `rung` (R,) int32 is updated in place, the temperatures swap with it.  parity
        None = round & 1.  With per-replica boxes the volumes are get_boxes() ** 3 and `pressure`
        enters; otherwise it is ignored.  Returns (attempt, accept), accumulated."""
        e, rung, res = self._ladder_arrays(n_rungs, energies, rung, attempt, accept)
        par = int(round) & 1 if parity is None else int(parity)
        check(self._L.mmc_batch_exchange(self._h, int(n_rungs), par, int(seed) & (2 ** 64 - 1), int(replica0),
                                         int(round), float(pressure), _d(e), _ptr(rung),
                                         *_ptrs(res, "attempt", "accept")))
        return res["attempt"], res["accept"]

    def run_exchange(self, n_rounds, steps_per_round, dr_max, dphi_max, seed, energies, rung, n_rungs, round0=0,
                     temperature=1.0, attempt=None, accept=None, n_groups=2, n_parts=0, time_kernels=False,
                     n_threads=1, n_streams=0, replica0=0):
        """mmc_batch_run_exchange: n_rounds x { steps_per_round trial moves of every replica at its
        own temperature, one exchange with round = round0 + i and parity = round & 1 }.  `rung` is
        updated in place.  `temperature` only has to be positive: the batch's array decides.
        Returns (energies, stats, attempt, accept)."""
        e, rung, res = self._ladder_arrays(n_rungs, energies, rung, attempt, accept)
        e = e.copy()
        p = RunParams(float(temperature), float(dr_max), float(dphi_max), int(seed), int(steps_per_round),
                      int(n_groups), int(n_parts), int(time_kernels), int(n_threads), int(n_streams), 0, int(replica0))
        st = RunStats()
        check(self._L.mmc_batch_run_exchange(self._h, C.byref(p), int(n_rounds), int(n_rungs), int(round0), _d(e),
                                             _ptr(rung), *_ptrs(res, "attempt", "accept"), C.byref(st)))
        return e, st.asdict(), res["attempt"], res["accept"]

    def widom(self, n_insert, temperature, seed, draw0=0, offsets=None, boltz_sum=None,
              n_overlap=None, outputs=False):
        """mmc_batch_widom: n_insert random insertions of the test molecule into every replica.
        offsets (3, 3) A from the COM, None = molecule 1 of the creating configuration
        (self.widom_offsets).  boltz_sum / n_overlap (R,) accumulate (new zero arrays when None).
        Returns (boltz_sum, n_overlap), and with outputs=True also mol (R, M, 12), du (R, M, 3)
        and ovl (R, M)."""
        off = _f64(self.widom_offsets if offsets is None else offsets).reshape(3, 3)
        M = int(n_insert)
        res = _insertion_outputs(self.R, M, boltz_sum, n_overlap, (12,) if outputs else None, outputs)
        check(self._L.mmc_batch_widom(self._h, M, int(seed) & (2 ** 64 - 1), int(draw0), _d(off),
                                      float(temperature), *_ptrs(res, "boltz_sum", "n_overlap", "mol", "du", "ovl")))
        return tuple(res.values())

    def widom_at(self, mol, temperature, boltz_sum=None, n_overlap=None):
        """mmc_batch_widom_at: the caller's test molecules mol (R, M, 12) = atoms (9), COM (3).
        Returns (boltz_sum, n_overlap, du (R, M, 3), ovl (R, M))."""
        mol = _f64(mol)
        if mol.ndim != 3 or mol.shape[0] != self.R or mol.shape[2] != 12:
            raise ValueError("mol must be (R, n_insert, 12)")
        M = mol.shape[1]
        res = _insertion_outputs(self.R, M, boltz_sum, n_overlap, None, True)
        check(self._L.mmc_batch_widom_at(self._h, M, _d(mol), float(temperature),
                                         *_ptrs(res, "boltz_sum", "n_overlap", "du", "ovl")))
        return tuple(res.values())

    def widom_solute(self, solute, n_insert, temperature, seed, draw0=0, boltz_sum=None, n_overlap=None,
                     outputs=False):
        """mmc_batch_widom_solute: n_insert random insertions of the foreign rigid solute
        (structs.Solute, S sites) into every replica, drawn as widom() draws its molecules: for one
        (seed, draw0) the reference points are widom()'s COMs.  boltz_sum / n_overlap (R,) accumulate
        (new zero arrays when None).  Returns (boltz_sum, n_overlap), and with outputs=True also mol
        (R, M, S + 1, 3) = the sites, then the reference point, du (R, M, 3) and ovl (R, M)."""
        S = solute.n_sites
        M = int(n_insert)
        res = _insertion_outputs(self.R, M, boltz_sum, n_overlap, (S + 1, 3) if outputs else None, outputs)
        check(self._L.mmc_batch_widom_solute(self._h, S, _d(solute.offsets), _d(solute.charge), _d(solute.eps),
                                             _d(solute.sig), M, int(seed) & (2 ** 64 - 1), int(draw0),
                                             float(temperature),
                                             *_ptrs(res, "boltz_sum", "n_overlap", "mol", "du", "ovl")))
        return tuple(res.values())

    def widom_solute_at(self, solute, mol, temperature, boltz_sum=None, n_overlap=None):
        """mmc_batch_widom_solute_at: the caller's solutes mol (R, M, S + 1, 3) = the S sites, then
        the reference point (the solute's offsets are not used).  Returns (boltz_sum, n_overlap,
        du (R, M, 3), ovl (R, M))."""
        S = solute.n_sites
        mol = _f64(mol)
        if mol.ndim != 4 or mol.shape[0] != self.R or mol.shape[2:] != (S + 1, 3):
            raise ValueError("mol must be (R, n_insert, n_sites + 1, 3)")
        M = mol.shape[1]
        res = _insertion_outputs(self.R, M, boltz_sum, n_overlap, None, True)
        check(self._L.mmc_batch_widom_solute_at(self._h, S, _d(solute.charge), _d(solute.eps), _d(solute.sig), M,
                                                _d(mol), float(temperature),
                                                *_ptrs(res, "boltz_sum", "n_overlap", "du", "ovl")))
        return tuple(res.values())

    # ---- a fixed solute (include/mmc_hip.h, "A fixed solute") ----
    def set_solute(self, solute, mol=None):
        """mmc_batch_set_solute: hold the rigid solute (structs.Solute) fixed in every replica at mol
        (S + 1, 3) = its S sites, then its reference point; every trial move, total and saved state
        then sees it as molecule N + 1.  solute None removes it.  A charged solute (set or removed)
        leaves S(k) stale: call recip_long() or potential_ewald() before the next run."""
        if solute is None:
            check(self._L.mmc_batch_set_solute(self._h, 0, None, None, None, None))
            return
        S = solute.n_sites
        mol = _f64(mol)
        if mol.shape != (S + 1, 3):
            raise ValueError("mol must be (n_sites + 1, 3): the sites, then the reference point")
        check(self._L.mmc_batch_set_solute(self._h, S, _d(mol), _d(solute.charge), _d(solute.eps), _d(solute.sig)))

    def _solute_sites(self):
        """The number of sites of the fixed solute, 0 while none is set."""
        n = C.c_int32(0)
        check(self._L.mmc_batch_get_solute(self._h, C.byref(n), None, None, None, None))
        return n.value

    def get_solute(self):
        """mmc_batch_get_solute: (structs.Solute, mol (S + 1, 3)) as set -- the Solute's offsets are the
        sites minus the reference point -- or None while no solute is set."""
        from .structs import Solute
        S = self._solute_sites()
        if S == 0:
            return None
        res = _outputs({"mol": ((S + 1, 3), np.float64), "charge": ((S,), np.float64), "eps": ((S, 3), np.float64),
                        "sig": ((S, 3), np.float64)}, None)
        check(self._L.mmc_batch_get_solute(self._h, None, *_ptrs(res, "mol", "charge", "eps", "sig")))
        return Solute("solute", res["mol"][:S] - res["mol"][S], res["charge"], res["eps"], res["sig"]), res["mol"]

    def solute_energy(self, out=None):
        """mmc_batch_solute_energy: the water-solute pair energy of every replica, the summand of
        <u_sw>: (u_lj (R,), u_real (R,), ovl (R,) uint8) in K; `out`: a dict of such arrays to write."""
        res = _outputs({"u_lj": ((self.R,), np.float64), "u_real": ((self.R,), np.float64),
                        "ovl": ((self.R,), np.uint8)}, out, known_only=True)
        check(self._L.mmc_batch_solute_energy(self._h, *_ptrs(res, "u_lj", "u_real", "ovl")))
        return res["u_lj"], res["u_real"], res["ovl"]

    def rdf_solute(self, numbins, r_max=0.0, per_replica=False, out=None):
        """mmc_batch_rdf_solute: solute-water pair histograms, uint64 [1 + S, 3, numbins] summed over
        the replicas or [R, 1 + S, 3, numbins] with per_replica: row 0 from the reference point, row
        1 + a from site a, against the three water slots; bin k holds k dr < r <= (k + 1) dr, dr as
        rdf_sites'.  `out` (that shape, uint64, contiguous) is overwritten and returned."""
        shape = (1 + self._solute_sites(), 3, max(int(numbins), 1))
        out = _output(out, (self.R,) + shape if per_replica else shape, np.uint64)
        check(self._L.mmc_batch_rdf_solute(self._h, int(numbins), float(r_max), int(bool(per_replica)), _ptr(out)))
        return out

    HYDRATION_CHANNELS = ("O", "H1", "H2", "px", "py", "pz", "u_lj", "u_real")

    def hydration_map(self, n_half, cell, channels=255, per_replica=False, out=None):
        """mmc_batch_hydration_map: the maps of the water around the fixed solute on a cube of
        (2 n_half)^3 cells of edge `cell` on the laboratory axes, centred on the solute's reference
        point.  `channels`: a mask (bit k = channel k) or an iterable of names among "O", "H1", "H2"
        (counts of the three water slots), "px", "py", "pz" (sums of the unit bisector's components
        in units of 2^-30, at the O's cell), "u_lj", "u_real" (sums of the water's pair energy with
        the solute in units of 2^-20 K, at the O's cell).  Returns int64 [n_ch, cells + 2], summed over
        the replicas, or [R, n_ch, cells + 2] with per_replica: the requested channels in rising bit
        order; slot `cells` holds the deposits outside the cube, slot cells + 1 the number of waters
        left out (no bisector; an overlap or an energy beyond 2^20 K).  observables.hydration_density,
        hydration_polarisation, hydration_energy and hydration_radial_average take its rows.  `out`
        (that shape, int64, contiguous) is overwritten and returned."""
        if isinstance(channels, (int, np.integer)):
            mask = int(channels)
        else:
            names = [channels] if isinstance(channels, str) else list(channels)
            unknown = [c for c in names if c not in self.HYDRATION_CHANNELS]
            if unknown:
                raise ValueError(f"channels: {unknown} are not among {self.HYDRATION_CHANNELS}")
            mask = sum({1 << self.HYDRATION_CHANNELS.index(c) for c in names})
        n = max(int(n_half), 0)
        cells = (2 * n) ** 3
        n_ch = bin(mask & 255).count("1")   # (arguments the library refuses still get an array to leave alone)
        shape = (n_ch, cells + 2)
        if out is None and cells > 16384:   # (a grid the library refuses: two slots a channel, not cells + 2)
            shape = (n_ch, 2)
        out = _output(out, (self.R,) + shape if per_replica else shape, np.int64)
        check(self._L.mmc_batch_hydration_map(self._h, int(n_half), float(cell), mask, int(bool(per_replica)), _ptr(out)))
        return out

    def solute_forces(self, details=False, out=None):
        """mmc_batch_solute_forces: what the water does to the fixed solute in every replica.  Returns a
        dict: force (R, 3) in K / A and torque (R, 3) in K about the reference point, flags (R,) uint8
        (bit 0: an overlap; bit 1: a non-finite output; a flagged replica's rows are zeros); with
        details also site_lj (R, S, 3), the Lennard-Jones force on every site, field (R, S, 3) in
        K / (e A) and phi (R, S) in K / e, the field and the potential at every site (phi = dU/dq_a; the
        force on site a is site_lj[a] + q_a field[a]), and recip (R, S, 4), the reciprocal part of
        (field, phi) alone.  `out`: a dict of such arrays to write.  Read-only."""
        R, S = self.R, self._solute_sites()
        spec = {"force": ((R, 3), np.float64), "torque": ((R, 3), np.float64)}
        if details:
            spec.update(site_lj=((R, S, 3), np.float64), field=((R, S, 3), np.float64), phi=((R, S), np.float64),
                        recip=((R, S, 4), np.float64))
        spec["flags"] = ((R,), np.uint8)
        res = _outputs(spec, out, known_only=True)
        check(self._L.mmc_batch_solute_forces(self._h, *_ptrs(res, "force", "torque", "site_lj", "field", "phi", "recip",
                                                               "flags")))
        return res

    def pair_sums(self, sums, K):
        """The six accumulators of widom_pair: a dict (or None = new zero arrays) with boltz_a (R,),
        n_zero_a (R,), boltz_b, boltz_ab (R, K), n_zero_b, n_zero_ab (R, K)."""
        f8, i8, one, per_d = np.float64, np.int64, (self.R,), (self.R, K)
        # (in the order mmc_batch_widom_pair and _pair_at take them)
        return _outputs({"boltz_a": (one, f8), "n_zero_a": (one, i8), "boltz_b": (per_d, f8), "n_zero_b": (per_d, i8),
                         "boltz_ab": (per_d, f8), "n_zero_ab": (per_d, i8)}, sums, where="sums")

    def widom_pair(self, pair, d, n_insert, temperature, seed, draw0=0, sums=None, outputs=False):
        """mmc_batch_widom_pair: n_insert random insertions of the solute pair (structs.SolutePair)
        into every replica, B at the K separations d (A) from A along one random ray per insertion;
        A is drawn as widom_solute() draws it.  `sums`: a dict of the six accumulators (pair_sums;
        None = new zero arrays), added to in place and returned: boltz_a, n_zero_a (R,), boltz_b,
        n_zero_b, boltz_ab, n_zero_ab (R, K).  With outputs=True also returns mol_a (R, M, S_A + 1,
        3), mol_b (R, M, K, S_B + 1, 3), du (R, M, 1 + 2 K, 3) = A, B_0.., x_0.. and flags (R, M,
        1 + K).  observables.pair_pmf turns the sums into g(d) and w(d)."""
        a, b = pair.a, pair.b
        d = _f64(d).ravel()
        K, M = d.shape[0], int(n_insert)
        R, sm = self.R, self.pair_sums(sums, K)
        spec = {}
        if outputs:
            spec = {"mol_a": ((R, M, a.n_sites + 1, 3), np.float64), "mol_b": ((R, M, K, b.n_sites + 1, 3), np.float64),
                    "du": ((R, M, 1 + 2 * K, 3), np.float64), "flags": ((R, M, 1 + K), np.uint8)}
        new = _outputs(spec, None)
        check(self._L.mmc_batch_widom_pair(
            self._h, a.n_sites, _d(a.offsets), _d(a.charge), _d(a.eps), _d(a.sig), b.n_sites, _d(b.offsets),
            _d(b.charge), _d(b.eps), _d(b.sig), _d(pair.eps_ab), _d(pair.sig_ab), K, _d(d), M,
            int(seed) & (2 ** 64 - 1), int(draw0), float(temperature), *_ptrs(sm, *sm),
            *_ptrs(new, "mol_a", "mol_b", "du", "flags")))
        return (sm, *new.values()) if outputs else sm

    def widom_pair_at(self, pair, mol_a, mol_b, temperature, sums=None):
        """mmc_batch_widom_pair_at: the caller's placements mol_a (R, M, S_A + 1, 3) and mol_b (R, M,
        K, S_B + 1, 3), sites then the reference point (offsets and separations are not used).
        Returns (sums, du (R, M, 1 + 2 K, 3), flags (R, M, 1 + K))."""
        a, b = pair.a, pair.b
        mol_a, mol_b = _f64(mol_a), _f64(mol_b)
        if mol_a.ndim != 4 or mol_a.shape[0] != self.R or mol_a.shape[2:] != (a.n_sites + 1, 3):
            raise ValueError("mol_a must be (R, n_insert, n_sites_a + 1, 3)")
        M = mol_a.shape[1]
        if mol_b.ndim != 5 or mol_b.shape[:2] != (self.R, M) or mol_b.shape[3:] != (b.n_sites + 1, 3):
            raise ValueError("mol_b must be (R, n_insert, n_sep, n_sites_b + 1, 3)")
        K = mol_b.shape[2]
        sm = self.pair_sums(sums, K)
        new = _outputs({"du": ((self.R, M, 1 + 2 * K, 3), np.float64), "flags": ((self.R, M, 1 + K), np.uint8)}, None)
        check(self._L.mmc_batch_widom_pair_at(
            self._h, a.n_sites, _d(a.charge), _d(a.eps), _d(a.sig), b.n_sites, _d(b.charge), _d(b.eps), _d(b.sig),
            _d(pair.eps_ab), _d(pair.sig_ab), K, M, _d(mol_a), _d(mol_b), float(temperature), *_ptrs(sm, *sm),
            *_ptrs(new, "du", "flags")))
        return sm, new["du"], new["flags"]

    def deletion(self, temperature, sel=None, bins=None, per_replica=False, boltz_sum=None,
                 n_flagged=None, details=False):
        """mmc_batch_deletion: the deletion (binding) energy dU_i = potential(N) - potential(N
        without i) of the molecules `sel` (0-based indices shared by all replicas, duplicates
        allowed; None = all N) of every replica, read-only.  bins = (n_bins, u_lo, u_hi) asks for
        the histogram of dU (observables.energy_bins' rule), summed over the replicas or one row
        each with per_replica.  boltz_sum float64 (R,) and n_flagged int64 (R,) accumulate
        sum exp(+dU / T) and the flagged molecules (new zero arrays when None).  Returns a dict:
        esum (R, 4) = sums of d_lj, d_real, d_recip and the number summed, boltz_sum, n_flagged,
        hist uint64 (n_bins + 2,) or (R, n_bins + 2) when bins is given, and with details=True du
        (R, n, 3) and ovl uint8 (R, n) (bit 0 overlap, bit 1 non-finite dU)."""
        R = self.R
        sel_a, n = _selection(sel, self.n_mol)
        spec = {"esum": ((R, 4), np.float64), "boltz_sum": ((R,), np.float64), "n_flagged": ((R,), np.int64)}
        n_bins, u_lo, u_hi = 0, 0.0, 0.0
        if bins is not None:
            n_bins, u_lo, u_hi = int(bins[0]), float(bins[1]), float(bins[2])
            slots = max(n_bins, 0) + 2   # (an n_bins the library refuses still gets an array to leave alone)
            spec["hist"] = ((R, slots) if per_replica else (slots,), np.uint64)
        if details:
            spec.update(du=((R, n, 3), np.float64), ovl=((R, n), np.uint8))
        res = _outputs(spec, dict(boltz_sum=boltz_sum, n_flagged=n_flagged), where=None)
        check(self._L.mmc_batch_deletion(
            self._h, n, None if sel_a is None else _ptr(sel_a), float(temperature), n_bins, u_lo, u_hi,
            int(bool(per_replica)), *_ptrs(res, "hist", "esum", "boltz_sum", "n_flagged", "du", "ovl")))
        return res

    def forces(self, sel=None, mass=None, details=False, n_flagged=None):
        """mmc_batch_forces: minus the gradient of potential(..., "ewald") at fixed neighbour sets on
        the atoms of the molecules `sel` (0-based indices shared by all replicas, duplicates allowed;
        None = all N) of every replica, read-only.  mass (3,) per atom slot asks for t = tau' I^-1 tau
        (else 0).  n_flagged int64 (R,) accumulates the flagged molecules (a new zero array when
        None).  Returns a dict: fsum (R, 9) = (number summed, sum F.F, sum tau.tau, sum t, sum F_x,
        sum F_y, sum F_z, sum w_lj, sum w_real), n_flagged, and with details=True force (R, n, 3),
        torque (R, n, 3), vir (R, n, 3) = (w_lj, w_real, t), atom (R, n, 3, 3) and ovl uint8 (R, n)
        (bit 0 overlap, bit 1 a non-finite output; a flagged molecule's rows are zeros)."""
        R = self.R
        sel_a, n = _selection(sel, self.n_mol)
        mass_a = None
        if mass is not None:
            mass_a = np.ascontiguousarray(mass, dtype=np.float64)
            if mass_a.shape != (3,):
                raise ValueError("mass: three values, one per atom slot")
        spec = {"fsum": ((R, 9), np.float64), "n_flagged": ((R,), np.int64)}
        if details:
            spec.update(force=((R, n, 3), np.float64), torque=((R, n, 3), np.float64), vir=((R, n, 3), np.float64),
                        atom=((R, n, 3, 3), np.float64), ovl=((R, n), np.uint8))
        res = _outputs(spec, dict(n_flagged=n_flagged), where=None)
        check(self._L.mmc_batch_forces(
            self._h, n, None if sel_a is None else _ptr(sel_a), None if mass_a is None else _d(mass_a),
            *_ptrs(res, "force", "torque", "vir", "atom", "fsum", "n_flagged", "ovl")))
        return res

    def get_trace(self, n_steps):
        """(dU[R, n], flags[R, n]) of the first n steps of the last run (option "trace_steps" = n):
        flags bit 0 accepted, bit 1 overlap, bit 2 rotation."""
        d = np.zeros((self.R, int(n_steps)))
        f = np.zeros((self.R, int(n_steps)), dtype=np.uint8)
        check(self._L.mmc_batch_get_trace(self._h, _d(d), _ptr(f)))
        return d, f

    def set_orientations(self, quat, db, faithful=True):
        """Turn on the reference's quaternion move generation for device-side proposals
        (mmc_batch_set_orientations): quat (n_mol, 4), db (3, 3) body-fixed sites; faithful keeps
        the reference's q_to_a including its (2,3) element.  quat=None turns it off."""
        if quat is None:
            check(self._L.mmc_batch_set_orientations(self._h, None, None, 0))
            return
        q, d = _f64(quat).reshape(self.n_mol, 4), _f64(db).reshape(3, 3)
        check(self._L.mmc_batch_set_orientations(self._h, _d(q), _d(d), 1 if faithful else 2))

    def get_orientations(self, r):
        q = np.empty((self.n_mol, 4))
        check(self._L.mmc_batch_get_orientations(self._h, int(r), _d(q)))
        return q

    def peek_part(self, r, part):
        """(64 raw bytes, stamp) of the result record of (replica r, part) of the last eval()."""
        buf = (C.c_uint8 * 64)()
        stamp = C.c_uint32()
        check(self._L.mmc_batch_peek_part(self._h, int(r), int(part), buf, C.byref(stamp)))
        return bytes(buf), stamp.value

    def part_validate(self, raw64, stamp):
        buf = (C.c_uint8 * 64).from_buffer_copy(raw64)
        return bool(self._L.mmc_part_validate(buf, int(stamp)))

    def rdf(self, site, numbins):
        """mmc_batch_rdf: histogram hist[0..numbins] of gr.jl's makeRDF over all replicas."""
        hist = np.zeros(int(numbins) + 1, dtype=np.uint64)
        check(self._L.mmc_batch_rdf(self._h, int(site), int(numbins), _ptr(hist)))
        return hist

    def rdf_sites(self, numbins, r_max=0.0, per_replica=False, out=None):
        """mmc_batch_rdf_sites: the six site-site pair histograms (observables.SLOT_PAIRS, each
        hist[0..numbins]) in one pass: uint64 [6, numbins + 1] summed over the replicas, or
        [R, 6, numbins + 1] with per_replica.  r_max <= 0: bins of (L / 2) / numbins (one shared
        box only), else of r_max / numbins.  `out` (that shape, uint64, contiguous) is overwritten
        and returned."""
        n1 = max(int(numbins), 0) + 1  # (a numbins the library refuses still gets an array to leave alone)
        out = _output(out, (self.R, 6, n1) if per_replica else (6, n1), np.uint64)
        check(self._L.mmc_batch_rdf_sites(self._h, int(numbins), float(r_max), int(bool(per_replica)), _ptr(out)))
        return out

    def dipoles(self, out=None):
        """mmc_batch_dipoles: the total dipole moment of every replica, [R, 3] in e A."""
        out = _output(out, (self.R, 3), np.float64)
        check(self._L.mmc_batch_dipoles(self._h, _ptr(out)))
        return out

    def orient_corr(self, numbins, r_max=0.0, per_replica=False, out=None):
        """mmc_batch_orient_corr: orientational pair correlations over the slot-0 separation, the
        bins of rdf_sites' row (0,0) plus slot numbins + 1 for every pair beyond r_max: int64
        [4, numbins + 2] summed over the replicas, or [R, 4, numbins + 2] with per_replica.  Row 0
        the pair count, rows 1..3 the sums of u_i.u_j, 3 (u_i.rhat)(u_j.rhat) - u_i.u_j and
        P2(u_i.u_j) in units of 2^-30 (observables.kirkwood_gk, orient_projections); u the unit
        vector of the molecule's dipole.  `out` (that shape, int64, contiguous) is overwritten and
        returned."""
        n2 = max(int(numbins), 0) + 2  # (a numbins the library refuses still gets an array to leave alone)
        out = _output(out, (self.R, 4, n2) if per_replica else (4, n2), np.int64)
        check(self._L.mmc_batch_orient_corr(self._h, int(numbins), float(r_max), int(bool(per_replica)), _ptr(out)))
        return out

    def sdf(self, n_half, cell, fold=3, site_mask=1, per_replica=False, out=None):
        """mmc_batch_sdf: the spatial distribution function's counts, the sites selected in
        site_mask (bit a = slot a) of every neighbour per cell of a cube of half-width n_half cell
        in the centre molecule's body-fixed frame (z the bisector, x in the molecular plane);
        fold bit 0 / 1 folds x / y onto |x| / |y|.  Returns Sdf(grid, outside, noframe): grid
        uint64 [g_x, g_y, g_z] with g = n_half along a folded axis and 2 n_half otherwise, the
        deposits outside the cube and those of centres without a frame; summed over the replicas
        or with a leading [R] axis with per_replica (observables.sdf_density, sdf_unfold,
        sdf_cell_centres).  `out` (uint64 [g_x g_y g_z + 2] or [R, g_x g_y g_z + 2], contiguous:
        the library's layout) is overwritten, and the results are views of it."""
        n, f = max(int(n_half), 0), int(fold)  # (arguments the library refuses still get an array to leave alone)
        g = (n if f & 1 else 2 * n, n if f & 2 else 2 * n, 2 * n)
        cells = g[0] * g[1] * g[2]
        shape = (self.R, cells + 2) if per_replica else (cells + 2,)
        if out is None and cells > 32768:   # (a grid the library refuses: two slots to leave alone, not cells + 2)
            out = np.zeros(shape[:-1] + (2,), dtype=np.uint64)
        else:
            out = _output(out, shape, np.uint64)
        check(self._L.mmc_batch_sdf(self._h, int(n_half), float(cell), f, int(site_mask), int(bool(per_replica)),
                                    _ptr(out)))
        return Sdf(out[..., :cells].reshape(shape[:-1] + g), out[..., cells], out[..., cells + 1])

    def pair_energy(self, numbins, r_max=0.0, n_ebins=0, u_lo=-4000.0, u_hi=2000.0, u_hb=None, per_replica=False,
                    out=None):
        """mmc_batch_pair_energy: the interaction energy u = u_C + u_LJ (K) of every pair of
        molecules whose slot-0 separation is in range, over orient_corr's bins.  Returns
        PairEnergy(rows, uhist, nhb, flagged), summed over the replicas or with a leading [R] axis
        with per_replica: rows int64 [3, numbins + 2], the pair count and the sums of u_C and u_LJ
        in units of 2^-20 K (observables.pair_energy_profile); uhist uint64 [n_ebins + 2], the
        pairs in range binned on u over [u_lo, u_hi) by observables.energy_bins' rule, None with
        n_ebins = 0 (observables.pair_energy_distribution); nhb uint64 [9], the molecules with
        0..7 and 8 or more partners below u_hb, None with u_hb = None
        (observables.energetic_hbonds); flagged uint64 [1], the pairs in range whose u_C or u_LJ
        is not finite or beyond 2^20 K, which enter row 0 only.  `out`: a dict of arrays under
        those names to overwrite instead (each of its shape and dtype, contiguous)."""
        R, n2, ne = self.R, max(int(numbins), 0) + 2, int(n_ebins)
        lead = (R,) if per_replica else ()
        spec = {"rows": (lead + (3, n2), np.int64), "flagged": (lead if per_replica else (1,), np.uint64)}
        if ne != 0:   # (an n_ebins the library refuses still gets an array to leave alone)
            spec["uhist"] = (lead + (max(ne, 0) + 2,), np.uint64)
        if u_hb is not None:
            spec["nhb"] = (lead + (9,), np.uint64)
        res = _outputs(spec, out, known_only=True)
        check(self._L.mmc_batch_pair_energy(
            self._h, int(numbins), float(r_max), ne, float(u_lo), float(u_hi),
            0.0 if u_hb is None else float(u_hb), int(bool(per_replica)),
            *_ptrs(res, "rows", "uhist", "nhb", "flagged")))
        return PairEnergy(res["rows"], res.get("uhist"), res.get("nhb"), res["flagged"])

    def structure_factor(self, n_max, per_replica=False, out=None):
        """mmc_batch_structure_factor: the products rho_a(n) rho_b(n)* of the three atom-slot
        densities over the box's own wave vectors q = 2 pi n / L, 0 < |n|^2 <= n_max^2, summed per
        shell s = |n|^2.  Returns (count, sq): count int32 [n_max^2 + 1], the vectors of each shell;
        sq int64 [R, 6, n_max^2 + 1] in units of 2^-24 with per_replica, else float64
        [6, n_max^2 + 1] summed over the replicas; rows observables.SLOT_PAIRS, a row (a, b), a < b,
        holding the cross term once (observables.partial_structure_factors,
        charge_structure_factor).  `out` (sq's shape and dtype, contiguous) is overwritten and
        returned.  With per-replica boxes only per_replica=True."""
        S = max(int(n_max), 0) ** 2 + 1  # (an n_max the library refuses still gets arrays to leave alone)
        shape, dt = ((self.R, 6, S), np.int64) if per_replica else ((6, S), np.float64)
        out = _output(out, shape, dt)
        count = np.zeros(S, dtype=np.int32)
        check(self._L.mmc_batch_structure_factor(self._h, int(n_max), int(bool(per_replica)), _ptr(count),
                                                 _ptr(out) if per_replica else None,
                                                 None if per_replica else _ptr(out)))
        return count, out

    def local_order(self, q_bins=400, r_hb=3.5, theta_deg=30.0, per_replica=False, details=False, out=None):
        """mmc_batch_local_order: hydrogen bonds (O-O closer than r_hb, H-O...O angle within
        theta_deg) and the tetrahedral order parameter q of every molecule (slot 0 = O, slots 1, 2
        = H).  Returns a dict: hb_hist uint64 [3, 9] (rows donated, accepted, total; molecules with
        n = 0..8), q_hist uint64 [q_bins] over [-3, 1] -- each [R, ...] with per_replica -- and
        q_sum [R, 2] (sum of the replica's finite q, their number).  details=True adds nbr int32
        [R, N, 4] (the four nearest, by rank), q [R, N] and hb uint8 [R, N, 2] (donated, accepted).
        `out`: a dict of arrays under those names to overwrite instead (each of its shape and
        dtype, contiguous)."""
        R, N, nq = self.R, self.n_mol, max(int(q_bins), 0)
        lead = (R,) if per_replica else ()
        spec = {"hb_hist": (lead + (3, 9), np.uint64), "q_hist": (lead + (nq,), np.uint64),
                "q_sum": ((R, 2), np.float64)}
        if details:
            spec.update(nbr=((R, N, 4), np.int32), q=((R, N), np.float64), hb=((R, N, 2), np.uint8))
        res = _outputs(spec, out)
        check(self._L.mmc_batch_local_order(
            self._h, float(r_hb), float(np.cos(np.deg2rad(float(theta_deg)))), int(q_bins),
            int(bool(per_replica)), *_ptrs(res, "hb_hist", "q_hist", "q_sum", "nbr", "q", "hb")))
        return res

    def shell_order(self, r_list=6.0, r_lsi=3.7, r_ang=3.3, r_hb=3.5, theta_deg=30.0, n_rank=8, r_bins=300,
                    lsi_bins=200, lsi_max=0.4, ang_bins=180, zeta_bins=200, zeta_lo=-1.5, zeta_hi=2.5,
                    per_replica=False, details=False, out=None):
        """mmc_batch_shell_order: every molecule's O-O neighbours inside r_list sorted by distance,
        and from that list the order between the first and second shell (slot 0 = O, slots 1, 2 = H),
        read-only.  Returns a dict: rank_hist uint64 [n_rank, r_bins + 1] (row k - 1: the distance to
        the k-th neighbour in bins of r_list / r_bins; last slot: fewer than k listed), lsi_hist
        uint64 [lsi_bins + 1] (the local structure index over [0, lsi_max] with r_lsi; last slot:
        undefined), ang_hist uint64 [ang_bins + 1] (cos of the O-O-O angles between neighbours
        inside r_ang over [-1, 1]; last slot: not finite), zeta_hist uint64 [zeta_bins + 1] (zeta
        over [zeta_lo, zeta_hi] with local_order's bonds of (r_hb, theta_deg); last slot: undefined)
        -- each [R, ...] with per_replica -- flagged uint64 [R] (molecules with more than 64
        neighbours inside r_list: in no histogram) and sums [R, 4] (sum of the replica's defined
        LSI, their number, sum of its defined zeta, their number).  details=True adds count int32
        [R, N] (listed neighbours, -1 where flagged), nbr int32 [R, N, 16] (the nearest 16 by rank,
        then -1), lsi and zeta [R, N] (NaN where undefined).  `out`: a dict of arrays under those
        names to overwrite instead (each of its shape and dtype, contiguous)."""
        R, N = self.R, self.n_mol
        nk, nr, nl, na, nz = (max(int(v), 0) for v in (n_rank, r_bins, lsi_bins, ang_bins, zeta_bins))
        lead = (R,) if per_replica else ()
        # (sizes the library refuses still get arrays to leave alone)
        spec = {"rank_hist": (lead + (nk, nr + 1), np.uint64), "lsi_hist": (lead + (nl + 1,), np.uint64),
                "ang_hist": (lead + (na + 1,), np.uint64), "zeta_hist": (lead + (nz + 1,), np.uint64),
                "flagged": ((R,), np.uint64), "sums": ((R, 4), np.float64)}
        if details:
            spec.update(count=((R, N), np.int32), nbr=((R, N, 16), np.int32), lsi=((R, N), np.float64),
                        zeta=((R, N), np.float64))
        res = _outputs(spec, out)
        check(self._L.mmc_batch_shell_order(
            self._h, float(r_list), float(r_lsi), float(r_ang), float(r_hb),
            float(np.cos(np.deg2rad(float(theta_deg)))), int(n_rank), int(r_bins), int(lsi_bins), float(lsi_max),
            int(ang_bins), int(zeta_bins), float(zeta_lo), float(zeta_hi), int(bool(per_replica)),
            *_ptrs(res, "rank_hist", "lsi_hist", "ang_hist", "zeta_hist", "flagged", "sums", "count", "nbr", "lsi",
                   "zeta")))
        return res

    def voronoi(self, r_list=7.0, area_min=0.0, v_bins=200, v_max=80.0, eta_bins=200, eta_max=3.0, r_bins=280,
                per_replica=False, details=False, out=None):
        """mmc_batch_voronoi: the Voronoi cell of every molecule's O from its O-O neighbours inside
        r_list (at most 64, at most half the smallest box), read-only.  Returns a dict: vol_hist
        uint64 [v_bins + 1] (cell volume over [0, v_max); last slot: beyond), eta_hist uint64
        [eta_bins + 1] (asphericity S^3 / (36 pi V^2) over [1, eta_max); last slot: beyond), face_hist
        uint64 [65] (molecules by their number of counted faces: those with area > area_min),
        side_hist uint64 [17] (counted faces by number of sides), nbr_hist uint64 [r_bins + 1] (O-O
        distance of counted faces over [0, r_list)) -- each [R, ...] with per_replica -- flagged
        uint64 [R, 3] (molecules with more than 64 neighbours in range; whose cell is not certified
        closed inside the list; whose polygon passed 16 vertices: in no histogram and no sum) and sums
        [R, 8] (number summed, sum V, sum V^2, sum S, sum eta, sum of counted faces, sum of their
        area, 0).  details=True adds vol and area [R, N] (NaN where flagged), faces int32 [R, N]
        (counted faces, or minus the flag bits), nbr int32 [R, N, 64] (the geometric neighbours by
        rank, then -1) and face_area [R, N, 64] (their face areas, then 0).  `out`: a dict of arrays
        under those names to overwrite instead (each of its shape and dtype, contiguous)."""
        R, N = self.R, self.n_mol
        nv, ne, nr = (max(int(v), 0) for v in (v_bins, eta_bins, r_bins))
        lead = (R,) if per_replica else ()
        # (sizes the library refuses still get arrays to leave alone)
        spec = {"vol_hist": (lead + (nv + 1,), np.uint64), "eta_hist": (lead + (ne + 1,), np.uint64),
                "face_hist": (lead + (65,), np.uint64), "side_hist": (lead + (17,), np.uint64),
                "nbr_hist": (lead + (nr + 1,), np.uint64), "flagged": ((R, 3), np.uint64), "sums": ((R, 8), np.float64)}
        if details:
            spec.update(vol=((R, N), np.float64), area=((R, N), np.float64), faces=((R, N), np.int32),
                        nbr=((R, N, 64), np.int32), face_area=((R, N, 64), np.float64))
        res = _outputs(spec, out)
        check(self._L.mmc_batch_voronoi(
            self._h, float(r_list), float(area_min), int(v_bins), float(v_max), int(eta_bins), float(eta_max),
            int(r_bins), int(bool(per_replica)),
            *_ptrs(res, "vol_hist", "eta_hist", "face_hist", "side_hist", "nbr_hist", "flagged", "sums", "vol", "area",
                   "faces", "nbr", "face_area")))
        return res

    def bond_order(self, l=3, r_nb=3.5, n_nb=4, a=(-np.inf, -0.8), b=(-0.35, 0.25), min_a=3, min_ab=4, q_bins=200,
                   c_bins=200, per_replica=False, details=False, out=None):
        """mmc_batch_bond_order: Steinhardt's q_l (l = 3, 4 or 6) of every molecule over its n_nb
        nearest O-O neighbours inside r_nb, the neighbour-averaged qbar_l, the bond correlations
        c_ij = q_l(i) . q_l(j)* / (|q_l(i)| |q_l(j)|), the bonds in the closed windows a and b
        (defaults: CHILL+'s staggered (-inf, -0.8] and eclipsed [-0.35, 0.25]) and the clusters of
        solid-like molecules (defined, at least min_a bonds in a and min_ab in a and b together),
        read-only.  Returns a dict: q_hist and qbar_hist uint64 [q_bins + 1] over [0, 1] and c_hist
        uint64 [c_bins + 1] over [-1, 1] per directed bond (last slot: undefined), ab_hist uint64
        [17, 17] (defined molecules at [n_a, n_b]), size_hist uint64 [N + 1] (solid clusters by
        size) -- each [R, ...] with per_replica -- stats int64 [R, 8] (defined, undefined, flagged,
        truncated, solid molecules, solid clusters, the largest, the sum of s^2) and sums [R, 4] (sum
        of the replica's defined q_l, their number, sum of its defined qbar_l, their number).
        details=True adds q and qbar [R, N] (NaN where undefined), nbr int32 [R, N, 16] (the
        neighbours used, by rank, then -1), ab uint8 [R, N, 2] (n_a, n_b) and label int32 [R, N] (the
        lowest index of the molecule's cluster, -1 if not solid).  `out`: a dict of arrays under
        those names to overwrite instead (each of its shape and dtype, contiguous)."""
        R, N = self.R, self.n_mol
        nq, nc = (max(int(v), 0) for v in (q_bins, c_bins))
        lead = (R,) if per_replica else ()
        # (sizes the library refuses still get arrays to leave alone)
        spec = {"q_hist": (lead + (nq + 1,), np.uint64), "qbar_hist": (lead + (nq + 1,), np.uint64),
                "c_hist": (lead + (nc + 1,), np.uint64), "ab_hist": (lead + (17, 17), np.uint64),
                "size_hist": (lead + (N + 1,), np.uint64), "stats": ((R, 8), np.int64), "sums": ((R, 4), np.float64)}
        if details:
            spec.update(q=((R, N), np.float64), qbar=((R, N), np.float64), nbr=((R, N, 16), np.int32),
                        ab=((R, N, 2), np.uint8), label=((R, N), np.int32))
        res = _outputs(spec, out)
        check(self._L.mmc_batch_bond_order(
            self._h, int(l), float(r_nb), int(n_nb), float(a[0]), float(a[1]), float(b[0]), float(b[1]), int(min_a),
            int(min_ab), int(q_bins), int(c_bins), int(bool(per_replica)),
            *_ptrs(res, "q_hist", "qbar_hist", "c_hist", "ab_hist", "size_hist", "stats", "sums", "q", "qbar", "nbr",
                   "ab", "label")))
        return res

    def hbond_network(self, r_hb=(3.5,), theta_deg=(30.0,), min_bonds=(0,), per_replica=False, details=False,
                      out=None):
        """mmc_batch_hbond_network: the hydrogen-bond graph of every replica under K = 1..8 criteria
        at once (bond: local_order's geometry with r_hb[k], theta_deg[k]; sites: the molecules with
        at least min_bonds[k] bonds; scalars are broadcast), read-only.  Returns a dict: size_hist
        uint64 [K, N + 1] (clusters by number of sites), deg_hist uint64 [K, 17] (molecules by number
        of bonds) -- each [R, ...] with per_replica -- and stats int64 [R, K, 8]: bonds, sites,
        clusters, the largest cluster, the sum of s^2, the OR of the wrap masks (x = 1, y = 2, z = 4),
        the largest wrapping cluster, flagged (some molecule with more than 16 bonds: all else 0).
        details=True adds label int32 [R, K, N] (the lowest index of the molecule's cluster, -1 off
        the sites, -2 where flagged) and nbr int32 [R, K, N, 16] (the bonded partners, ascending, then
        -1).  `out`: a dict of arrays under those names to overwrite instead (each of its shape and
        dtype, contiguous)."""
        R, N = self.R, self.n_mol
        crit = np.broadcast_arrays(np.atleast_1d(_f64(r_hb)), np.atleast_1d(_f64(theta_deg)),
                                   np.atleast_1d(np.asarray(min_bonds)))
        if crit[0].ndim != 1:
            raise ValueError("r_hb, theta_deg and min_bonds are scalars or 1-D of one length")
        rh = np.ascontiguousarray(crit[0], dtype=np.float64)
        cs = np.ascontiguousarray(np.cos(np.deg2rad(crit[1])), dtype=np.float64)
        mb = np.ascontiguousarray(crit[2], dtype=np.int32)
        if not np.array_equal(mb, crit[2]):
            raise ValueError("min_bonds must be integers")
        K = rh.shape[0]
        lead = (R,) if per_replica else ()
        spec = {"size_hist": (lead + (K, N + 1), np.uint64), "deg_hist": (lead + (K, 17), np.uint64),
                "stats": ((R, K, 8), np.int64)}
        if details:
            spec.update(label=((R, K, N), np.int32), nbr=((R, K, N, 16), np.int32))
        res = _outputs(spec, out)
        check(self._L.mmc_batch_hbond_network(
            self._h, K, _d(rh), _d(cs), _ptr(mb), int(bool(per_replica)),
            *_ptrs(res, "size_hist", "deg_hist", "stats", "label", "nbr")))
        return res

    def hbond_rings(self, r_hb=3.5, theta_deg=30.0, n_max=8, per_replica=False, details=False, max_rings=0, out=None):
        """mmc_batch_hbond_rings: the shortest-path rings (Franzblau) of 3 .. n_max <= 8 molecules in
        the hydrogen-bond graph of every replica under one criterion (hbond_network's bond with r_hb,
        theta_deg), read-only.  Returns a dict: ring_hist uint64 [3, 9] (by size: the rings that do
        not wrap the box, those that do, the homodromic ones among the first), member_hist uint64
        [9, 33] (row n: molecules by the number of n-rings they are in, row 0 by rings of any size,
        last bin 32 or more) -- each [R, ...] with per_replica -- and stats int64 [R, 8]: bonds,
        rings, wrapping rings, homodromic rings, molecules in no ring, the most rings one molecule
        is in, rings that did not fit into `ring`, flagged (some molecule with more than 8 bonds: all
        else 0).  details=True adds count uint16 [R, N, 9] (per molecule the rings of each size,
        entry 0 their total; 65535 where flagged) and, with max_rings > 0, ring int32
        [R, max_rings, 8]: the rings in canonical form (lowest member, the smaller of its two ring
        neighbours, onward), padded with -1, in no particular order.  `out`: a dict of arrays under
        those names to overwrite instead (each of its shape and dtype, contiguous)."""
        R, N = self.R, self.n_mol
        lead = (R,) if per_replica else ()
        spec = {"ring_hist": (lead + (3, 9), np.uint64), "member_hist": (lead + (9, 33), np.uint64),
                "stats": ((R, 8), np.int64)}
        if details:
            spec["count"] = ((R, N, 9), np.uint16)
            if int(max_rings) > 0:
                spec["ring"] = ((R, int(max_rings), 8), np.int32)
        res = _outputs(spec, out)
        check(self._L.mmc_batch_hbond_rings(
            self._h, float(r_hb), float(np.cos(np.deg2rad(float(theta_deg)))), int(n_max), int(bool(per_replica)),
            *_ptrs(res, "ring_hist", "member_hist", "stats", "count"), int(max_rings), *_ptrs(res, "ring")))
        return res

    def _cavity(self, points, n_probe, seed, draw0, radii, site, n_cap, nn_bins, nn_max, per_replica, details):
        R, P = self.R, max(int(n_probe), 0)
        rad = _f64(np.atleast_1d(radii)).ravel()
        K, cap, nb = rad.shape[0], max(int(n_cap), 0), max(int(nn_bins), 0)
        lead = (R,) if per_replica else ()
        # (sizes the library refuses still get arrays to leave alone)
        spec = {"occ_hist": (lead + (K, cap + 1), np.uint64), "occ_mom": (lead + (K, 2), np.uint64)}
        if nb > 0:
            spec["nn_hist"] = (lead + (nb + 1,), np.uint64)
            if nn_max is None:
                raise ValueError("nn_bins > 0 needs nn_max")
        if details:
            if points is None:
                spec["points"] = ((R, P, 3), np.float64)
            spec.update(count=((R, P, K), np.int32), nn_r2=((R, P), np.float64), nn_idx=((R, P), np.int32))
        res = _outputs(spec, None)
        common = (int(site), K, _d(rad), int(n_cap), nb, float(nn_max) if nb > 0 else 0.0, int(bool(per_replica)),
                  *_ptrs(res, "occ_hist", "occ_mom", "nn_hist"))
        tail = _ptrs(res, "count", "nn_r2", "nn_idx")
        if points is None:
            check(self._L.mmc_batch_cavity(self._h, int(n_probe), int(seed) & (2 ** 64 - 1), int(draw0), *common,
                                           *_ptrs(res, "points"), *tail))
        else:
            check(self._L.mmc_batch_cavity_at(self._h, int(n_probe), _d(points), *common, *tail))
            if details:
                res["points"] = points
        return res

    def cavity(self, n_probe, seed, draw0=0, radii=(3.3,), site=0, n_cap=32, nn_bins=0, nn_max=None,
               per_replica=False, details=False):
        """mmc_batch_cavity: n_probe random points in every replica (bit for bit the COMs widom draws
        for the same seed and draw0), read-only.  For each radius (1..8, ascending, A) the number n
        of sites -- atom slot `site` of every molecule, or the centres of mass with site = -1 --
        closer than it to a point.  Returns a dict: occ_hist uint64 [K, n_cap + 1] (points with
        n = 0 .. n_cap; the last bin stands for n_cap or more), occ_mom uint64 [K, 2] (the sums of n
        and n^2, unclamped) and, with nn_bins > 0, nn_hist uint64 [nn_bins + 1]: the distance of the
        nearest site in bins of nn_max / nn_bins, the last for nn_max and beyond
        (observables.cavity_size_distribution) -- each [R, ...] with per_replica.  details=True adds
        points [R, n_probe, 3], count int32 [R, n_probe, K], nn_r2 [R, n_probe] and nn_idx int32
        [R, n_probe]."""
        return self._cavity(None, n_probe, seed, draw0, radii, site, n_cap, nn_bins, nn_max, per_replica, details)

    def cavity_at(self, points, radii=(3.3,), site=0, n_cap=32, nn_bins=0, nn_max=None, per_replica=False,
                  details=False):
        """mmc_batch_cavity_at: as cavity(), at the caller's points (R, n_probe, 3)."""
        points = _f64(points)
        if points.ndim != 3 or points.shape[0] != self.R or points.shape[2] != 3:
            raise ValueError("points must be (R, n_probe, 3)")
        return self._cavity(points, points.shape[1], 0, 0, radii, site, n_cap, nn_bins, nn_max, per_replica, details)

    def volume_perturb(self, temperature, scales=None, dv=None, boltz_sum=None, n_overlap=None, details=False):
        """mmc_batch_volume_perturb: virtual volume moves of every replica, read-only.  Test boxes
        L_k = scales[k] L (1..8 of them), or volume changes dv (A^3) converted by
        ((V + dv) / V) ** (1 / 3) (volumeChange.jl:60).  boltz_sum float64 (R, K) and n_overlap int64
        (R, K) accumulate w = exp(-dU / T + N ln(scale^3)) and the weights forced to 0 (new zero
        arrays when None).  Returns (boltz_sum, n_overlap), and with details=True also du (R, K, 4) =
        (dLJ, dreal, drecip, dself) and base (R, 4), the parts of the energy at f = 1
        (observables.pressure_from_volume_perturbation turns the sums into a pressure)."""
        if (scales is None) == (dv is None):
            raise ValueError("give either scales or dv")
        if scales is None:
            v = self.box ** 3
            sc = np.array([((v + float(x)) / v) ** (1.0 / 3.0) for x in np.atleast_1d(dv)])
        else:
            sc = _f64(np.atleast_1d(scales)).ravel()
        K = sc.shape[0]
        spec = {"boltz_sum": ((self.R, K), np.float64), "n_overlap": ((self.R, K), np.int64)}
        if details:
            spec.update(du=((self.R, K, 4), np.float64), base=((self.R, 4), np.float64))
        res = _outputs(spec, dict(boltz_sum=boltz_sum, n_overlap=n_overlap), where=None)
        check(self._L.mmc_batch_volume_perturb(self._h, K, _d(sc), float(temperature),
                                               *_ptrs(res, "boltz_sum", "n_overlap", "du", "base")))
        return tuple(res.values())

    # ---- save and resume (include/mmc_hip.h, "Save and resume"; checkpoint.py) ----
    def state_info(self):
        """mmc_batch_state_info: the _lib.StateInfo of the batch as it is configured now."""
        info = _lib.StateInfo()
        check(self._L.mmc_batch_state_info(self._h, C.byref(info)))
        return info

    def get_state(self, r0=0, nr=None, out=None):
        """mmc_batch_get_state: the records of replicas [r0, r0 + nr) (nr None: to the last) as a uint8
        array [nr, record_bytes], the caller's `out` or a new one.  Changes nothing."""
        from . import checkpoint
        r0 = int(r0)
        nr = self.R - r0 if nr is None else int(nr)
        if not (0 <= r0 <= self.R and 0 <= nr <= self.R - r0):
            raise ValueError(f"replicas [{r0}, {r0 + nr}) outside 0..{self.R}")
        rb = checkpoint.record_layout(self.state_info())[1]
        out = _output(out, (nr, rb), np.uint8)
        check(self._L.mmc_batch_get_state(self._h, r0, nr, out.ctypes.data_as(C.c_void_p)))
        return out

    def set_state(self, info, records, r0=0):
        """mmc_batch_set_state: `records` (uint8 [nr, record_bytes], as get_state returns them) into
        replicas [r0, r0 + nr).  `info` (state_info() of the batch that wrote them, or the dict of a
        checkpoint's header) must agree with this batch's system and with how it is configured now."""
        from . import checkpoint
        sinfo = info if isinstance(info, _lib.StateInfo) else checkpoint.info_from_dict(info)
        rb = checkpoint.record_layout(sinfo)[1]
        if not (isinstance(records, np.ndarray) and records.dtype == np.uint8 and records.ndim == 2
                and records.shape[1] == rb and records.flags.c_contiguous):
            raise ValueError(f"records: a C-contiguous uint8 array of shape (nr, {rb})")
        r0, nr = int(r0), records.shape[0]
        if not (0 <= r0 <= self.R and nr <= self.R - r0):
            raise ValueError(f"replicas [{r0}, {r0 + nr}) outside 0..{self.R}")
        check(self._L.mmc_batch_set_state(self._h, C.byref(sinfo), r0, nr, records.ctypes.data_as(C.c_void_p)))

    _SOLUTE_EXTRA = ("solute_mol", "solute_charge", "solute_eps", "solute_sig")   # save()'s own names among `extra`

    def save(self, path, extra=None, replica0=0):
        """Write the batch's state to the checkpoint file `path` (checkpoint.py), atomically.  `extra`:
        a dict of the numpy arrays the caller holds and the batch does not -- running energies, the
        chains array of run_chains, rung / attempt / accept and the exchange round, NPT statistics.
        `replica0`: the global index of this batch's first replica (a rank saves its own shard).
        Options are not saved: the resuming batch sets them, as at creation."""
        from . import checkpoint
        info = self.state_info()
        sol = self.get_solute()
        taken = sorted(set(extra or {}) & set(self._SOLUTE_EXTRA))
        if taken:
            raise ValueError(f"extra: the names {taken} are the file's own (the batch's solute); choose others")
        if sol is not None:   # (the arrays mmc_state_info::solute_hash is the fingerprint of: load() sets them again)
            extra = dict(extra or {}, solute_mol=sol[1], solute_charge=sol[0].charge, solute_eps=sol[0].eps,
                         solute_sig=sol[0].sig)
        rb = checkpoint.record_layout(info)[1]
        per = max(1, min(self.R, checkpoint.CHUNK_BYTES // rb))
        buf = np.zeros((per, rb), dtype=np.uint8)
        checkpoint.write(path, info, self.R, lambda r0, n: self.get_state(r0, n, out=buf[:n]), extra=extra,
                         replica0=replica0, chunk_records=per)

    def load(self, path):
        """Resume from the checkpoint `path`, written by save() of a batch of the same system and
        size; this batch may have been created from any coordinates.  Refuses, before anything reaches
        the library's state, a wrong magic or version, a truncated file, a CRC mismatch and a state of
        another system.  Then brings the batch into the saved mode through its own setters
        (set_coulomb_style, set_boxes, volume_change, set_temperatures, set_orientations, set_solute)
        and streams the records in with set_state.  Returns the file's `extra` arrays.  Chains continue bit for
        bit when this batch has the options (kernel, parts, persistent / server_wgs,
        steps_per_launch, half_k) of the one that saved."""
        from . import checkpoint
        head = checkpoint.read_header(path)
        saved = head["info"]
        if saved["n_mol"] != self.n_mol:
            raise checkpoint.CheckpointError(f"identity mismatch: the checkpoint's n_mol is {saved['n_mol']}, the "
                                             f"batch has {self.n_mol}")
        if head["n_records"] != self.R:
            raise checkpoint.CheckpointError(f"identity mismatch: the checkpoint holds {head['n_records']} replicas, "
                                             f"the batch has {self.R}")
        boxes, temps = checkpoint.verify(path, head)        # every CRC, before the batch is touched
        mine = checkpoint.info_to_dict(self.state_info())
        checkpoint.check_identity(saved, mine)
        same_solute = (saved.get("solute_on", 0), saved.get("solute_hash", 0)) == (mine.get("solute_on", 0),
                                                                                   mine.get("solute_hash", 0))
        # (first: a solute fences the setters below -- also the detour through Wolf style that marks a fresh
        # S(k) stale as saved; the solute is then set again at the end)
        stale_by_wolf = (saved["coulomb_style"] == 0 and saved["s_stale"]
                         and not (mine["coulomb_style"] == 0 and mine["s_stale"]))
        if mine.get("solute_on", 0) and (not same_solute or stale_by_wolf or saved["coulomb_style"] != 0
                                           or saved["per_box"] or saved["box"] != mine["box"]
                                           or saved["kappa"] != mine["kappa"]):
            self.set_solute(None)
            same_solute = not saved.get("solute_on", 0)
            mine = checkpoint.info_to_dict(self.state_info())
        style = self.COULOMB_STYLES[saved["coulomb_style"]]
        if style == "wolf":
            self.set_coulomb_style("wolf")
        elif saved["s_stale"] and not (mine["coulomb_style"] == 0 and mine["s_stale"]):
            self.set_coulomb_style("wolf")                   # (back from Wolf: S(k) awaits its rebuild, as saved)
            self.set_coulomb_style("ewald")
        else:
            self.set_coulomb_style("ewald")
            if mine["s_stale"] or mine["coulomb_style"] != 0:
                self.recip_long()
        if saved["per_box"]:
            self.set_boxes(boxes, saved["alpha"])
        elif mine["per_box"]:
            raise checkpoint.CheckpointError("the checkpoint has one box, the batch per-replica boxes, which cannot be "
                                             "switched off: create a new batch")
        elif saved["box"] != mine["box"] or saved["kappa"] != mine["kappa"]:
            self.volume_change(saved["box"], saved["kappa"])
        self.set_temperatures(temps if saved["temps_on"] else None)
        if saved["quat_mode"]:   # (any unit quaternions: the records bring the saved ones)
            self.set_orientations(np.tile([1.0, 0.0, 0.0, 0.0], (self.n_mol, 1)), saved["db"],
                                  faithful=saved["quat_mode"] == 1)
        elif mine["quat_mode"]:
            self.set_orientations(None, None)
        extra = checkpoint.read_extra(path, head)
        if saved.get("solute_on", 0) and not same_solute:
            from .structs import Solute
            mol = extra["solute_mol"]
            self.set_solute(Solute("solute", mol[:-1] - mol[-1], extra["solute_charge"], extra["solute_eps"],
                                   extra["solute_sig"]), mol)
            if not saved["s_stale"] and self.state_info().s_stale:
                self.recip_long()                            # (a charged solute: S(k) awaits no rebuild, as saved)
        extra = {k: v for k, v in extra.items() if k not in self._SOLUTE_EXTRA}
        sinfo = checkpoint.info_from_dict(saved)
        for r0, rec in checkpoint.iter_chunks(path, head):
            self.set_state(sinfo, rec, r0)
        return extra

    def new_chains(self, energies, virials=None, dr_max=0.15, dphi_max=0.05, set_value=0.5):
        """One mmc_chain record per replica (numpy structured array, _lib.CHAIN_DTYPE): the
        bookkeeping Loop() keeps in total / averages / trans_moves / rot_moves / totProps."""
        c = np.zeros(self.R, dtype=CHAIN_DTYPE)
        c["dr_max"], c["dphi_max"] = dr_max, dphi_max
        c["energy"] = energies
        c["virial"] = 0.0 if virials is None else virials
        c["trans_set_value"] = c["rot_set_value"] = set_value
        return c

    def run_chains(self, chains, n_steps, temperature, seed, adjust=True, n_groups=2, n_parts=0,
                   time_kernels=False, n_threads=1, n_streams=0, replica0=0):
        """mmc_batch_run_chains: `chains` (from new_chains) is updated in place."""
        if chains.dtype != CHAIN_DTYPE or chains.shape != (self.R,) or not chains.flags.c_contiguous:
            raise ValueError("chains must be the array returned by new_chains()")
        p = RunParams(float(temperature), 0.0, 0.0, int(seed), int(n_steps), int(n_groups),
                      int(n_parts), int(time_kernels), int(n_threads), int(n_streams), 0,
                      int(replica0))
        st = RunStats()
        check(self._L.mmc_batch_run_chains(self._h, C.byref(p), chains.ctypes.data_as(C.c_void_p),
                                           int(bool(adjust)), C.byref(st)))
        return st.asdict()
