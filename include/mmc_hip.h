/*
 * mmc_hip.h -- C ABI of libmmc_hip.so: the MI355X (gfx950) implementation of the per-move energy
 * hot path of BradenDKelly/MetropolisMonteCarlo.
 *
 * The reference has no FFI layer: its boundary is the set of Julia generic functions that
 * `Loop()` (Ewald/main.jl:460-696) and `potential()` (Ewald/energy.jl:946-1032) call.  Each entry
 * point below names the reference method it replaces (file:line into /root/reference).  The Julia
 * methods of the same names that `ccall` these symbols are in
 * metropolismontecarlo_amd/julia/MMCHip.jl and INTEGRATION.md; the Python mirror used by the
 * tests is metropolismontecarlo_amd/api.py.
 *
 * Conventions (what a `ccall` passes):
 *   - every array is a Julia Vector of bits types, borrowed for the duration of the call only:
 *       Vector{SVector{3,Float64}}  -> const double*  (3 doubles per element, x y z)
 *       Vector{Float64}             -> const double*
 *       Vector{Int64}               -> const int64_t* (atom ranges / types are 1-BASED, inclusive)
 *       Vector{SVector{3,Int32}}    -> int32_t*       (3 per element)
 *       Vector{ComplexF64}          -> double*        (re, im interleaved)
 *       Matrix{Float64}             -> const double*  (column-major n_types x n_types)
 *   - molecule indices (`i`, `chosenOne`) are 1-BASED as in the reference;
 *   - every function returns an int32 status (MMC_OK == 0); results come back through
 *     out-pointers; the library never calls exit() (the reference does, energy.jl:426-428);
 *   - a reference `@assert` becomes MMC_ERR_ASSERT; mmc_last_error() has the text;
 *   - one context (or batch) is not thread-safe, like the reference's mutable EWALD; different
 *     contexts may be driven from different threads and run on different HIP streams.
 * All arithmetic is fp64.  Energies are in K, lengths in Angstrom, charges in e.
 */
#ifndef MMC_HIP_H
#define MMC_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    MMC_OK = 0,
    MMC_ERR_ARG = 1,      /* null pointer, bad size, index out of range */
    MMC_ERR_ASSERT = 2,   /* a reference @assert would have thrown */
    MMC_ERR_HIP = 3,      /* a HIP runtime call failed (no device, OOM, launch failure) */
    MMC_ERR_STATE = 4,    /* call order: e.g. RecipMove before PrepareEwaldVariables */
    MMC_ERR_UNSUPPORTED = 5
};

typedef struct mmc_ctx mmc_ctx;     /* one system (one Markov chain) resident on one GPU */
typedef struct mmc_batch mmc_batch; /* R independent replicas of one system on one GPU   */

/* Totals written by the total-energy drivers: the fields of `Properties`
 * (Ewald/auxillary.jl:37-45) that potential() fills, plus the four terms it println()s. */
typedef struct {
    double energy, virial, coulomb;
    double lj, real, recip, self;
    int32_t n_overlap; /* molecules for which EwaldReal returned (0.0, true) */
    int32_t _pad;
} mmc_totals;

const char *mmc_last_error(void); /* thread-local text of the last non-OK status */
const char *mmc_version(void);
int32_t mmc_device_count(int32_t *count);

/* ---- context ------------------------------------------------------------------------------- */
/* `hip_stream`: a hipStream_t to launch on (e.g. torch.cuda.current_stream().cuda_stream), or
 * NULL to let the context own a non-blocking stream. */
int32_t mmc_ctx_create(int32_t device, void *hip_stream, mmc_ctx **out);
int32_t mmc_ctx_destroy(mmc_ctx *ctx);
int32_t mmc_ctx_synchronize(mmc_ctx *ctx);

/* Mirror moa/soa/vdwTable on the device.  Replaces nothing in the reference -- it is the price of
 * a device: the fields are exactly those LJ_poly_dU / EwaldReal read (Ewald/energy.jl:216-229,
 * Ewald/ewalds.jl:305-308): moa.COM, moa.firstAtom, moa.lastAtom, soa.coords, soa.atype,
 * soa.charge, vdwTable.eps_ij, vdwTable.sig_ij (Ewald/structs.jl:337-347), box. */
int32_t mmc_upload_system(mmc_ctx *ctx, int64_t n_mol, int64_t n_atoms, const double *com,
                          const int64_t *first_atom, const int64_t *last_atom,
                          const double *coords, const int64_t *atype, const double *charge,
                          int64_t n_types, const double *eps, const double *sig, double box);
/* Loop() writes the moved molecule into moa.COM[i] / soa.coords[first:last] before it calls the
 * energy functions (Ewald/main.jl:527,552) and restores them on rejection (:623-624); this is the
 * device-side counterpart of those two assignments.  `atoms`: 3*(last-first+1) doubles.
 * The context compares with its host mirror of the coordinates: an unchanged molecule costs nothing,
 * a changed one travels with the next evaluation instead of a launch of its own. */
int32_t mmc_set_molecule(mmc_ctx *ctx, int64_t i, const double *com, const double *atoms);
/* Re-send every centre of mass and atom position (same topology): the whole-array form of the
 * assignments above, for callers that changed more than one molecule on the host.  `com` may be
 * NULL to re-send the atoms only (all that RecipLong reads). */
int32_t mmc_update_system(mmc_ctx *ctx, const double *com, const double *coords);
int32_t mmc_download_system(mmc_ctx *ctx, double *com, double *coords);
/* The device part of an NPT volume move.  The reference only specifies it in prose
 * (Ewald/volumeChange.jl:59-80): centres of mass scale by new_box/box, atoms translate rigidly
 * with their molecule; then everything that depends on the box is rebuilt -- kappa (alpha/L,
 * Ewald/main.jl:290-291), kxyz/cfac (PrepareEwaldVariables, Ewald/ewalds.jl:45-103), zeroed
 * sumQExp arrays.  Follow with mmc_potential_ewald for the energy at the new volume
 * (volumeChange.jl:91-111). */
int32_t mmc_volume_change(mmc_ctx *ctx, double new_box, double new_kappa);
/* One NPT volume move without a host round trip (Ewald/volumeChange.jl:59-147, `MC_vol`).
 * mmc_volume_trial: copies aside ON THE DEVICE everything the move rewrites (coordinates in their
 * three layouts, fixed-point centres of mass, S(k), k-vectors, erfc table; one launch), then does
 * mmc_volume_change + mmc_potential_ewald: `tot` is the energy at the new volume (:91-111).
 * mmc_volume_accept (:132-147): nothing left to do.  mmc_volume_reject: the copy back (one
 * launch): coordinates, tables and S(k) are the pre-move ones bit for bit. */
int32_t mmc_volume_trial(mmc_ctx *ctx, double new_box, double new_kappa, double lj_rcut,
                         double qq_rcut, mmc_totals *tot);
int32_t mmc_volume_accept(mmc_ctx *ctx);
int32_t mmc_volume_reject(mmc_ctx *ctx);

/* PrepareEwaldVariables(ewald, boxSize)                       Ewald/ewalds.jl:45-103
 * Builds kxyz/cfac on the device, zeroes sumQExpOld/New.  k_sq_max != 27 -> MMC_ERR_ASSERT (:49).
 * `factor` is EWALD.factor (Ewald/constants.jl:24-28). */
int32_t mmc_prepare_ewald(mmc_ctx *ctx, double kappa, int64_t nk, int64_t k_sq_max, double box,
                          double factor, int64_t *nkvecs);
int32_t mmc_get_kvectors(mmc_ctx *ctx, int32_t *kxyz /* [NKVECS][3] */, double *cfac);
/* EWALD.sumQExpOld / sumQExpNew (Ewald/ewalds.jl:16-17); either pointer may be NULL. */
int32_t mmc_get_sumqexp(mmc_ctx *ctx, double *sum_old, double *sum_new);
int32_t mmc_set_sumqexp(mmc_ctx *ctx, const double *sum_old, const double *sum_new);

/* How the per-molecule calls are served.  Loop() calls LJ_poly_dU(i) and EwaldShort(i) in pairs on
 * an unchanged system (Ewald/main.jl:491+501, :557+566).  The context evaluates BOTH terms in one
 * command whichever is asked for first (the cutoff of the other term is assumed to be the one last
 * used for it, else the same) and answers the second call from that result without touching the
 * device -- valid as long as molecule, cutoffs and coordinates (a version number of the host
 * mirror) are unchanged.  For systems of identical 3-site molecules with an EWALD the evaluations
 * run on a persistent kernel (csrc/mmc_ctxsrv.hpp) that the host talks to through a command block
 * in pinned memory: no launch, no stream synchronisation per call; every wait is bounded, and the
 * kernel is stopped before anything else runs on the context (and after ~1 s without a call).
 * Other systems pay one launch per evaluation.  Results of the two paths agree to ~1e-13
 * relative (summation order; the server takes erfc(kappa r)/r from the table of the batch
 * kernels).
 *
 * LJ_poly_dU(i, moa, soa, vdwTable, r_cut, box)               Ewald/energy.jl:209-290
 * (and the legacy LJ_poly_dU(i, system::Requirements)          Ewald/energy.jl:126-206)
 * -> (4*pot, 24*vir/3). */
int32_t mmc_lj_poly_du(mmc_ctx *ctx, int64_t i, double r_cut, double *pot, double *vir);

/* EwaldReal(chosenOne, moa, soa, ewald, r_cut, box)           Ewald/ewalds.jl:293-376, ovr = 0.5
 * EwaldReal(qq_r, qq_q, kappa, box, thisMol_thisAtom, i, sys) Ewald/ewalds.jl:205-289, ovr = 1.0
 * -> (pot, overlap); pot WITHOUT factor; overlap -> pot = 0.0 (:359-360). */
int32_t mmc_ewald_real(mmc_ctx *ctx, int64_t i, double r_cut, double ovr, double *pot,
                       int32_t *overlap);

/* EwaldShort(i, moa, soa, sim_props, ewald, box)              Ewald/ewalds.jl:892-910
 * -> (e = EwaldReal*factor, e/3, overlap) with r_cut = sim_props.qq_rcut. */
int32_t mmc_ewald_short(mmc_ctx *ctx, int64_t i, double qq_rcut, double *e, double *v,
                        int32_t *overlap);

/* CoulombReal(qq_r, qq_q, box, chosenOne, system)             Ewald/energy.jl:618-711
 * bare Coulomb: COM gate r_cut + (r_cut*0.25+5), ovr = 1, atomic cutoff r2 < r_cut^2;
 * r_cut != 10.0 -> MMC_ERR_ASSERT (:648). */
int32_t mmc_coulomb_real(mmc_ctx *ctx, int64_t i, double r_cut, double *pot, int32_t *overlap);

/* RecipLong(ewald, r, qq_q, box)                              Ewald/ewalds.jl:538-604
 * (legacy RecipLong(system, ewald, r, qq_q)                    Ewald/ewalds.jl:465-534)
 * Full structure factor of the uploaded atoms; writes BOTH sumQExpOld and sumQExpNew (:600-601);
 * energy WITHOUT factor (:603). */
int32_t mmc_recip_long(mmc_ctx *ctx, double *energy);

/* RecipMove(box, ewalds, r_old, r_new, qq_q)                  Ewald/ewalds.jl:718-826
 * n != 3, k_sq_max != 27 or nk != 5 -> MMC_ERR_ASSERT (:740-743).  sumQExpNew += dS in place
 * (:805-814); returns energy*factor (:825). */
int32_t mmc_recip_move(mmc_ctx *ctx, const double *r_old, const double *r_new, const double *q,
                       int64_t n, double *d_energy);

/* ewald.sumQExpOld = copy(ewald.sumQExpNew)                   Ewald/main.jl:621
 * (on the device the two arrays are names of buffers: a commit or rollback renames, nothing is copied) */
int32_t mmc_recip_commit(mmc_ctx *ctx);
/* ewald.sumQExpNew = copy(ewald.sumQExpOld)                   Ewald/main.jl:628 */
int32_t mmc_recip_rollback(mmc_ctx *ctx);

/* ---- the same calls with the CALLER'S OWN ARRAYS: what a Julia method forwards --------------------
 * One ccall per reference call, nothing to keep in step by hand.  `com` / `coords` are moa.COM and
 * soa.coords (legacy: system.rm and qq_r / system.ra) as they are NOW, whole arrays.  Loop() changes
 * one molecule between calls and may have restored the one of the previous call (main.jl:527,552,
 * 623-624): the context looks at molecule i and at the molecule of its previous mmc_call_*, compares
 * them with its mirror, and sends what changed along with the evaluation.  After any other edit of
 * the arrays call mmc_update_system.
 *
 * mmc_call_recip_move takes ewalds.sumQExpOld / sumQExpNew as they are now.  Loop() rebinds them to
 * copies on every move (main.jl:621,628), so the context finds out which of its device buffers
 * each array is by CONTENT, against pinned host copies of those buffers (two 5.4 KB comparisons
 * on the host; arrays it has never seen are uploaded).  When the moved molecule was evaluated by
 * mmc_call_lj_poly_du / mmc_call_ewald_short while the device still held its old coordinates,
 * RecipMove was computed in that same command: the call then only checks r_old / r_new / q and the
 * arrays and copies sumQExpNew out.  sum_new is updated in place like the reference's
 * (ewalds.jl:805-814); d_energy has the factor applied (:825). */
int32_t mmc_call_lj_poly_du(mmc_ctx *ctx, int64_t i, const double *com, const double *coords,
                            double r_cut, double *pot, double *vir);
int32_t mmc_call_ewald_real(mmc_ctx *ctx, int64_t i, const double *com, const double *coords,
                            double r_cut, double ovr, double *pot, int32_t *overlap);
int32_t mmc_call_ewald_short(mmc_ctx *ctx, int64_t i, const double *com, const double *coords,
                             double qq_rcut, double *e, double *v, int32_t *overlap);
int32_t mmc_call_recip_move(mmc_ctx *ctx, const double *r_old, const double *r_new,
                            const double *q, int64_t n, const double *sum_old, double *sum_new,
                            double *d_energy);
/* Counters of the context: out[0..9] = commands answered by the persistent kernel, launches of it,
 * commands that had to be repeated on a fresh one, per-molecule calls answered from the cached
 * evaluation, RecipMoves answered from the speculative sum, speculative sums that went unused,
 * evaluations by ordinary launch, 1 if the persistent kernel is running, evaluations answered by
 * the look-ahead (the command that evaluates a moved molecule i also has molecule i + 1 -- the next
 * of Loop()'s sweep, main.jl:490 -- evaluated by a second set of workgroups; valid if nothing
 * changes before it is asked for, i.e. the move was accepted), look-aheads posted. */
int32_t mmc_ctx_stats(mmc_ctx *ctx, int64_t out[10]);
/* Test hook / measurement: average round trip in microseconds of n empty commands through the
 * running persistent kernel -- the floor under every served call. */
int32_t mmc_ctx_ping(mmc_ctx *ctx, int64_t n, double *us_avg);
/* "server": 1 (default) = use the persistent kernel when it applies, 0 = a launch per evaluation */
int32_t mmc_ctx_set_option(mmc_ctx *ctx, const char *key, int64_t value);

/* EwaldSelf(ewald, qq_q)                                      Ewald/ewalds.jl:829-833 (factor in) */
int32_t mmc_ewald_self(mmc_ctx *ctx, double *self_energy);

/* potential(moa, soa, tot, ewalds, vdwTable, sim_props, "ewald")   Ewald/energy.jl:946-1032
 * lj_rcut = sim_props.LJ_rcut, qq_rcut = sim_props.qq_rcut.  Takes everything from the context
 * (the reference reads globals `ewald`, `totProps`, :994 -- identical at its only call site). */
int32_t mmc_potential_ewald(mmc_ctx *ctx, double lj_rcut, double qq_rcut, mmc_totals *tot);
/* potential(moa, soa, tot, ewald, vdwTable, sim_props)  ("Wolf")  Ewald/energy.jl:864-943 */
int32_t mmc_potential_wolf(mmc_ctx *ctx, double lj_rcut, double qq_rcut, mmc_totals *tot);

/* The five hot-path calls of one Loop() iteration in ONE launch   Ewald/main.jl:491-593
 * (2x LJ_poly_dU, 2x EwaldShort, RecipMove) for molecule i moved to com_new/atoms_new.
 * d[0] = E_new_LJ - E_old_LJ, d[1] = real new - old (factor in), d[2] = deltaRecip (0 when
 * overlap, :580-590), d[3] = virial new - old + deltaRecip/3 (:600-601).  The device state is
 * left OLD; follow with mmc_accept_move (:598-621) or mmc_reject_move (:622-629). */
int32_t mmc_trial_move(mmc_ctx *ctx, int64_t i, const double *com_new, const double *atoms_new,
                       double lj_rcut, double qq_rcut, double d[4], int32_t *overlap);
int32_t mmc_accept_move(mmc_ctx *ctx);
int32_t mmc_reject_move(mmc_ctx *ctx);

/* ---- single-precision tolerance study (BASELINE.json configs[4]: Wolf vs Ewald, fp32 vs fp64) ---
 * Not a reference interface: the reference is fp64 only.  The same terms as mmc_lj_poly_du /
 * mmc_ewald_real / mmc_recip_long / mmc_recip_move, evaluated from coordinates rounded to fp32 with
 * fp32 arithmetic; mixed = 0: fp32 accumulators, 1: fp64 accumulators.
 * total: out = { LJ energy, LJ virial, real-space Coulomb (factor in), reciprocal (factor in),
 *                number of overlapping molecules, 0 } -- the summed terms of potential()
 *        (energy.jl:946-1032); add mmc_ewald_self for the Ewald total or the Wolf constants of
 *        mmc_potential_wolf (.self) for the Wolf total.  Also builds the fp32 structure factor.
 * move:  d = { dLJ, dReal, dRecip } of mmc_trial_move's d[0..2] in fp32 for molecule i (1-based)
 *        moved to com_new / atoms_new; the device state is not touched. */
int32_t mmc_study_f32_total(mmc_ctx *ctx, double lj_rcut, double qq_rcut, int32_t mixed,
                            double out[6]);
int32_t mmc_study_f32_move(mmc_ctx *ctx, int64_t i, const double *com_new, const double *atoms_new,
                           double lj_rcut, double qq_rcut, int32_t mixed, double d[3],
                           int32_t *overlap);

/* ---- replica batch: R independent NVT chains of the same system on one GPU ------------------ */
typedef struct {
    int32_t mol;         /* 1-based molecule index of this replica's trial move */
    int32_t accept_prev; /* 1: the PREVIOUS proposal of this replica was accepted -> commit it
                            (Ewald/main.jl:598-621) before evaluating; 0: discard it (:622-629) */
    double com_new[3];   /* moa.COM[i] after the move            (Ewald/main.jl:527) */
    double atoms_new[9]; /* soa.coords[first:last] after the move (Ewald/main.jl:552) */
} mmc_move;

typedef struct {
    double d_lj;    /* partial_new_e - partial_old_e, LJ part     (Ewald/main.jl:491,557) */
    double d_real;  /* EwaldShort new - old, factor applied       (Ewald/main.jl:501,566) */
    double d_recip; /* RecipMove, factor applied; 0 when overlap  (Ewald/main.jl:580-590) */
    double d_vir;   /* virial new - old + d_recip/3               (Ewald/main.jl:600-601) */
    int32_t overlap;
    int32_t _pad;
} mmc_move_result;

/* All replicas start from the given configuration (3 atoms per molecule required: RecipMove's
 * `@assert n == 3`, Ewald/ewalds.jl:740).  Ewald tables are prepared as mmc_prepare_ewald does;
 * call mmc_batch_recip_long once before the first mmc_batch_eval. */
int32_t mmc_batch_create(int32_t device, void *hip_stream, int64_t n_replicas, int64_t n_mol,
                         const double *com, const double *coords, const int64_t *atype,
                         const double *charge, int64_t n_types, const double *eps,
                         const double *sig, double box, double kappa, int64_t nk,
                         int64_t k_sq_max, double factor, double lj_rcut, double qq_rcut,
                         mmc_batch **out);
int32_t mmc_batch_destroy(mmc_batch *b);
int32_t mmc_batch_set_replica(mmc_batch *b, int64_t r, const double *com, const double *coords);
int32_t mmc_batch_get_replica(mmc_batch *b, int64_t r, double *com, double *coords,
                              double *sum_old);
/* RecipLong for every replica; energies[r] WITHOUT factor. */
int32_t mmc_batch_recip_long(mmc_batch *b, double *energies);
/* potential(..., "ewald") for every replica. */
int32_t mmc_batch_potential_ewald(mmc_batch *b, mmc_totals *tot);
/* ---- Coulomb style: the reference's global `Wolf` (Ewald/main.jl:75) for the batch's chains ----
 * A call of its own, not an option: options change nothing but summation order, the style changes
 * the chain.  The default is MMC_COULOMB_EWALD, and a batch that never sets a style is what it
 * always was.  In MMC_COULOMB_WOLF style mmc_batch_eval, _settle, _run and _run_chains take the
 * reference's Wolf move (main.jl:491-593 with `Wolf = true`): d_lj, d_real and overlap as in Ewald
 * style, no RecipMove (main.jl:580-590) -- d_recip = 0, d_vir = virial new - old without a
 * d_recip/3 term, dU = d_lj + d_real for the host's decision, the kernel's own and the
 * "trace_steps" hook.  Neither S(k) buffer of any replica is read or written
 * (mmc_batch_get_replica's sum_old is bit for bit what it was), and the proposals are those of
 * Ewald style: the same random streams at the same counters.  Every move kernel (options kernel 0,
 * 1, 2, 3) has its own Wolf instantiation without phase tables, k loop or S(k) traffic; with
 * "parts" > 1 every part is a pair part.
 * Switching needs no proposals outstanding (MMC_ERR_STATE).  Switching from Wolf back to Ewald
 * marks S(k) stale: until mmc_batch_recip_long (or mmc_batch_potential_ewald, which rebuilds S(k)
 * itself) has run, mmc_batch_eval, _run, _run_chains and _widom* return MMC_ERR_STATE.
 * Outside the Wolf style's scope, MMC_ERR_UNSUPPORTED with nothing computed and no state changed,
 * whichever call comes first: per-replica boxes (mmc_batch_set_boxes), every volume-move entry
 * point (mmc_batch_volume_*, mmc_batch_run_npt, mmc_batch_run_npt_replicas), mmc_batch_widom and
 * _widom_at, option "kernel" = 4 and option "persistent" = 1 ("persistent" = -1 uses launches). */
enum { MMC_COULOMB_EWALD = 0, MMC_COULOMB_WOLF = 1 };
int32_t mmc_batch_set_coulomb_style(mmc_batch *b, int32_t style);
int32_t mmc_batch_get_coulomb_style(mmc_batch *b, int32_t *style);
/* potential() of the Wolf overload (Ewald/energy.jl:864-943) for every replica, as
 * mmc_potential_wolf: lj = half the double-counted LJ sum, real = factor/2 x the EwaldReal sum with
 * NO virial term (:919-920), recip = 0, self = (prefactor - prefactor2) factor with r_cut = lj_rcut
 * (:875, :924-932; the double loop in closed form), n_overlap as mmc_batch_potential_ewald.  Same
 * preconditions as that call, and one more: the batch's one shared box (MMC_ERR_UNSUPPORTED after
 * mmc_batch_set_boxes).  Works in either style and does not touch S(k).
 * The virial of a Wolf CHAIN is not this total's: Loop() adds EwaldShort's virial e/3 per accepted
 * move (main.jl:566-568, :600-601) while this potential() adds none for the real part, so a chain's
 * running virial (mmc_chain.virial) changes as `virial + real / 3` of this call does, and a chain
 * that is to agree with a recompute starts from that sum. */
int32_t mmc_batch_potential_wolf(mmc_batch *b, mmc_totals *tot);
/* mmc_volume_change for every replica of the batch (they share one box). */
int32_t mmc_batch_volume_change(mmc_batch *b, double new_box, double new_kappa);
/* An NPT volume move of a ONE-replica batch without a host round trip -- the batch-side twin of
 * mmc_volume_trial / accept / reject, so that the trial moves of an NPT chain run on the batch's
 * fast paths (the move server: BASELINE configs[3], 10 000 molecules) and its volume moves on
 * the same state (the reference's only statement of the move: the docstring
 * Ewald/volumeChange.jl:59-147).  Trial: everything the move rewrites is copied aside on the device,
 * the system rescaled about the centres of mass (:62-80), the tables rebuilt for new_kappa
 * (ewalds.jl:45-103) and the total energy at the new volume evaluated (:91-111).  Accept (:132-147):
 * nothing to do.  Reject: the copy back, bit for bit.  A batch has ONE box: independent NPT
 * replicas are one batch each (MMC_ERR_UNSUPPORTED for more than one replica). */
int32_t mmc_batch_volume_trial(mmc_batch *b, double new_box, double new_kappa, mmc_totals *tot);
int32_t mmc_batch_volume_accept(mmc_batch *b);
int32_t mmc_batch_volume_reject(mmc_batch *b);
/* One trial move per replica, one launch: moves[r] -> results[r].  moves[r].accept_prev settles
 * the replica's previous proposal first.  Synchronous. */
int32_t mmc_batch_eval(mmc_batch *b, const mmc_move *moves, mmc_move_result *results);
/* Workgroups per replica-move used by mmc_batch_eval (1..32; 1 = one workgroup does the whole
 * move, >1 = the molecule range is split and the last workgroup does the reciprocal part). */
int32_t mmc_batch_set_parts(mmc_batch *b, int32_t n_parts);
/* Tuning switches (no effect on results beyond summation order):
 *   "parts"            as mmc_batch_set_parts
 *   "kernel"           2 = one wavefront per trial move, persistent workgroups, erfc(kappa r)/r
 *                      table; 1 = one workgroup per trial move (LDS-tiled, same table);
 *                      3 = 2 for launches of at least 16 moves per compute unit, else 1 (default
 *                      when every molecule has the same atom types and charges); 0 = generic;
 *                      4 = the latency form (k_move_eval_lat): "parts" (4, 8, ... 128) are waves,
 *                      four to a workgroup, each pair part's molecules resident in the wave, three
 *                      lanes to a neighbour, the reciprocal sum split over 1..3 waves; the form the
 *                      move server takes for few replicas -- same chains bit for bit as that server
 *   "wave_wgs"         workgroups of a kernel-2 launch (0 = 5 per compute unit: what its 96 VGPRs and
 *                      31 KB of LDS let be resident)
 *   "inject_torn"      N > 0: the native driver corrupts its first N copies of result records
 *                      before checking them, as a torn PCIe write would (test hook: the check must
 *                      refuse them and read again; mmc_run_stats.torn_records counts them)
 *   "local_stage"      0 = mmc_batch_local_order, mmc_batch_shell_order and mmc_batch_cavity read the site
 *                      positions from device memory even where a replica's fit in LDS (default 1; the
 *                      path of systems too large to stage, same results: a test hook)
 *   "voronoi_prune"    0 = mmc_batch_voronoi clips every face against every listed plane instead of
 *                      stopping at the first one out of its reach (default 1; same bits, for timing)
 *   "zero_copy_moves"  1 = the kernel reads proposals from pinned host memory instead of an
 *                      H2D copy on the stream (lower latency for one replica, default 0)
 *   "device_moves"     1 = mmc_batch_run / mmc_batch_run_chains generate the trial moves on the
 *                      device (counter-based Philox4x32-10 keyed by seed + replica and the step
 *                      number; same move distributions as the host generator, a different random
 *                      stream): only one flag byte per replica and step crosses PCIe and no host
 *                      mirror of the coordinates is kept.  Default 0.
 *   "accept_on_device" who makes the Metropolis decision of a step of mmc_batch_run / _run_chains:
 *                      1 = the move kernel itself, where it can (device_moves, one part per move,
 *                      the wave kernel, no step-size adaptation): Metropolis(dU / T) && !overlap with
 *                      the same Philox uniform the host would take, its S-buffer bit and accept flag
 *                      kept in device memory for the next launch's commit, the decision sent along
 *                      in the result record (bit 31 of the stamp word) for the host's bookkeeping --
 *                      the same chains bit for bit, and a launch does not wait for the host's pass
 *                      over the previous launch's records.  0 = the host (its threads read every
 *                      record, decide, and write a flag byte per replica before the next launch:
 *                      ~50 ns per record and thread, hidden behind the other group's kernel while
 *                      there are about 8 threads per 32768-move launch).  -1 (default) = 1 where
 *                      a launch can take several steps ("steps_per_launch"), or where a host thread
 *                      would have more than 4096 records per launch to decide; else 0.
 *                      The record of a launch of several steps ("steps_per_launch") has three words:
 *                      the sum of dU over the accepted steps, the accepted | overlap << 32 masks
 *                      and the kinds of the moves.  It carries NO virial: such launches compute
 *                      none (mmc_batch_run_chains, which accumulates the virial, takes one step
 *                      per launch).
 *   "steps_per_launch" where the move kernel decides (above) and the caller asks for energies and
 *                      counts only (mmc_batch_run; not _run_chains, not the "trace_steps" hook), ONE
 *                      launch takes every replica of a group through this many consecutive steps
 *                      -- the same wave commits, evaluates and decides step after step, what one
 *                      step wrote and read is in the caches for the next -- and sends one record
 *                      per replica and launch: the sum of dU over its accepted steps and bit masks
 *                      (accepted, overlap, kind of move).  1, 2, 4, 8 or 16; 0 (default) = 8.  Same
 *                      chains bit for bit (counts, coordinates, S(k)); the running energies differ
 *                      from one step per launch by the order of a sum.  mmc_run_stats.launches
 *                      counts the launches.  1.43e8 against 1.31e8 moves/s (61440 chains of 750
 *                      molecules, one run of bench.py).  Launches this long (1.7 ms) want groups whose size is a multiple
 *                      of 5 * 4 * (compute units) replicas -- 5120 on MI355X: every wavefront the
 *                      kernel keeps resident then takes the same number of replicas.  In such a
 *                      launch a wave takes its first replica by its index, every further one from
 *                      a queue (one ticket per replica and launch): the waves of a launch do not
 *                      finish together, and the quick ones take more replicas.
 *   "whole_call"       where launches take several steps (above): 1 = a call of n steps takes
 *                      ONE launch per group of min(n, 32, molecules - 1) steps, and a longer call
 *                      launches of that many; 0 (default) = launches of "steps_per_launch".  Same
 *                      chains bit for bit; the running energies differ by the order of a sum.  For
 *                      comparison: at the bench's 20-step call one launch per group ran 4 % slower
 *                      than launches of eight (the last launch's tail is one 20-step unit long).
 *   "image_by_molecule" -1 (default) = the wave kernel takes the minimum image of an atom pair with
 *                      the image of its molecule's centre of mass where that is the reference's
 *                      vector1D bit for bit: moves made on the device (rigid), and
 *                      gate + 2 r_mol < box / 2 (r_mol: the largest atom-to-centre distance of
 *                      anything uploaded).  0 = never: the per-pair minimum image.
 *   "persistent"       the move server for small batches (device_moves = 1, kernel != 0, no
 *                      orientations, at most one replica per compute unit): mmc_batch_run /
 *                      mmc_batch_run_chains launch ONE kernel per call, a workgroup per replica
 *                      whose waves are the parts of the move; per step the host posts one 8-byte
 *                      control word per replica in pinned memory (sequence number, result stamp,
 *                      accept bit of the previous step) and reads one 64-byte result record -- no
 *                      launch, no copy.  The chain is bit-identical to the launch-per-step driver
 *                      with n_parts = the server's waves (ceil(molecules / 64) + 1, at most 8 -- 5 for
 *                      a single replica -- or mmc_run_params.n_parts when > 1).  Every device-side wait is bounded (3 s):
 *                      a host that stops talking gets MMC_ERR_HIP from the run, not a hung GPU.
 *                      -1 (default) = use it for up to 256 replicas (one per compute unit) when it applies, 0 = never,
 *                      1 = insist (MMC_ERR_UNSUPPORTED from the run when it cannot be used)
 *   "trace_steps"      test hook: see mmc_batch_get_trace
 *   "server_wgs"       workgroups per replica of the move server: -1 (default) = 4 while each has
 *                      a compute unit to itself (up to 64 replicas), else 2 -- or, for a system too large for that, as many as it takes for
 *                      every pair wave to hold at most 128 molecules (10 000 molecules: 21) --
 *                      while R x workgroups does not exceed the compute units; 0 = one workgroup
 *                      per replica (k_move_server_wave); 2..32 = that many (k_move_server_lat: each
 *                      workgroup polls the replica's control word itself and keeps its own copy
 *                      of its molecules)
 *   "server_stall_ms"  test hook: the driver sleeps this long before posting the control words of
 *                      step 2 (the server's bounded wait must end the run with MMC_ERR_HIP)
 *   "server_seq_offset" test hook: the control words' sequence numbers (24 bits, compared modulo
 *                      2^24 on both sides) start at this offset instead of 0
 * A run that fails half-way (a server that timed out, a HIP error) leaves accepted moves, S-buffer
 * parity and the caller's energies in doubt: the batch then returns MMC_ERR_STATE from
 * mmc_batch_run / run_chains / eval until EVERY replica has been set again
 * (mmc_batch_set_replica); recompute the energies (mmc_batch_potential_ewald) after that. */
int32_t mmc_batch_set_option(mmc_batch *b, const char *key, int64_t value);
/* The fast kernel's approximation of erfc(kappa r)/r (ewalds.jl:367) evaluated at n values of
 * r^2 in (0, 256): lets a test bound its error against an exact evaluation. */
int32_t mmc_batch_qq_table(mmc_batch *b, const double *r2, int64_t n, double *out);
/* mmc_batch_qq_table for replica `replica` of a batch with per-replica boxes: its own table and
 * kappa = alpha / boxes[replica] (mmc_batch_set_boxes).  On a one-box batch: the shared table.  An
 * out-of-range replica returns MMC_ERR_ARG, like the arguments mmc_batch_qq_table refuses. */
int32_t mmc_batch_qq_table_replica(mmc_batch *b, int64_t replica, const double *r2, int64_t n,
                                   double *out);
/* Radial-distribution histogram over every replica of the batch: the intent of Ewald/gr.jl
 * `makeRDF` with each replica as one frame.  One site per molecule -- site >= 0: that atom slot
 * (0 = the oxygens of water), site < 0: the centre of mass (gr.jl's cm mode); all pairs i < j,
 * gr.jl's minimum image (:75-80), bin = ceil(r / dr), dr = box / 2 / numbins (:5,87), counted
 * when bin <= numbins.  hist[0 .. numbins] (numbins + 1 counters). */
int32_t mmc_batch_rdf(mmc_batch *b, int32_t site, int32_t numbins, uint64_t *hist);
/* The reference's own move generation for device-side proposals ("device_moves"): orientations are
 * unit quaternions `totProps.quat[i]` and the atoms of a moved molecule are rebuilt from its
 * body-fixed sites, ra[a] = COM + MATMUL(q_to_a(ei), db[a]) (Ewald/main.jl:516-549;
 * quaternions.jl:11-50 q_to_a, :93-120 rotate_quaternion, :158-182 random_rotate_quaternion;
 * auxillary.jl:154-159 MATMUL).  quat: [n_mol][4] (w, x, y, z), given to every replica; db: [3][3]
 * body-fixed coordinates of the three sites.  mode 1 = q_to_a exactly as the reference has it,
 * including its element (2,3) `2*(q[2]*q[4] + q[1]*q[2])` (quaternions.jl:43; the Allen & Tildesley
 * original reads q[3]*q[4] + q[1]*q[2], so the reference's matrix is not orthogonal); mode 2 = the
 * Allen & Tildesley matrix; mode 0 = back to the default (the current atoms are translated /
 * rotated rigidly about the centre of mass, no quaternions kept).  A quaternion whose squared
 * norm is off by more than 1e-6 returns MMC_ERR_ASSERT (the reference prints and exit()s,
 * quaternions.jl:20-25).  An accepted move commits its quaternion (`totProps.quat[i] = ei`,
 * main.jl:619).  The coordinates given at creation are the caller's: the reference builds them
 * from the same quaternions (MakeAtomArrays, Ewald/setup.jl:447-537).  Modes 1 and 2 raise the
 * batch's bound on a site's distance from its centre of mass (which picks the kernels that take an
 * atom pair's minimum image from its molecules') to what any orientation can reach: max_a |db[a]|
 * in mode 2; max_a (|db[a]| + sqrt(2) |db[a].y|) in mode 1, whose element (2,3) adds up to
 * sqrt(2) |db[a].y| along z; both times (1 + 1e-5) for the 1e-6 norm tolerance.  The bound is
 * never lowered, mode 0 included. */
int32_t mmc_batch_set_orientations(mmc_batch *b, const double *quat, const double *db,
                                   int32_t mode);
int32_t mmc_batch_get_orientations(mmc_batch *b, int64_t r, double *quat);
/* Result hand-off check (test hook): 1 if the 64-byte move-result record at `part_out_64` carries
 * launch stamp `stamp` and a matching checksum, else 0. */
int32_t mmc_part_validate(const void *part_out_64, uint32_t stamp);
/* Copy the raw 64-byte result record of (replica r, part) of the last mmc_batch_eval and the
 * stamp of that launch (test hook for the hand-off check). */
int32_t mmc_batch_peek_part(mmc_batch *b, int64_t r, int32_t part, void *out64, uint32_t *stamp);
/* Test hook: with option "trace_steps" = N the native driver records, for the first N steps of a
 * run and every replica, dU = d_lj + d_real + d_recip (main.jl:593) and the decision -- bit 0
 * accepted, bit 1 overlap, bit 2 the move was a rotation.  delta, flags: [R][N]. */
int32_t mmc_batch_get_trace(mmc_batch *b, double *delta, uint8_t *flags);
/* Settle the last outstanding proposals without evaluating new ones. */
int32_t mmc_batch_settle(mmc_batch *b, const int32_t *accept);

/* Native host driver: the sequential accept/reject of Loop() (Ewald/main.jl:487-644) for every
 * replica, in C++ on the host, around mmc_batch_eval's kernel.  Sweeps molecules in order like
 * the reference (`for i = 1:numbers.molecules`, :490). */
typedef struct {
    double temperature;  /* K                                (Ewald/main.jl:62)  */
    double dr_max;       /* translation box width, Angstrom  (Ewald/main.jl:118) */
    double dphi_max;     /* max rotation angle, rad          (Ewald/main.jl:73)  */
    uint64_t seed;       /* key of the run's random streams: chain r draws from the stream
                            (seed, replica0 + r) -- see "Random streams" below */
    int64_t n_steps;     /* trial moves per replica to run */
    int32_t n_groups;    /* replica groups pipelined on separate streams (>=1) */
    int32_t n_parts;     /* workgroups per replica-move (0 = choose) */
    int32_t time_kernels;/* N > 0: bracket every Nth launch of a group with HIP events, the
                            (N/2 + 1)th of each window of N (stats.kernel_ms over
                            stats.timed_launches); 0: none */
    int32_t n_threads;   /* host threads sharing the groups (0 or 1 = the calling thread only) */
    int32_t n_streams;   /* HIP streams the groups are spread over; 0 = choose (one per group with
                            host proposals; two with "device_moves": the launches of the groups
                            overlap -- stats.kernel_ms then sums SPANS of launches that share the
                            GPU, not costs; 1 = every launch alone on the GPU) */
    int32_t _pad;
    uint64_t replica0;   /* global index of this batch's replica 0 (a rank that owns chains
                            [g0, g0 + R) of a larger ensemble passes g0): the RANDOM DRAWS of a
                            chain depend on (seed, global index) only.  Its energies also depend,
                            in the last bits, on the order its dU terms are summed in, which the
                            batch picks from its own size (kernel by launch size, parts per move,
                            move server up to 256 replicas): shardings that use the same
                            "kernel", n_parts and "persistent" / "server_wgs" on every rank
                            reproduce one another bit for bit; others agree to ~1e-13 per move
                            and may part ways at a Metropolis comparison eventually */
} mmc_run_params;

/* Random streams.  Device-side proposals ("device_moves"): every draw is Philox4x32-10 with key =
 * seed (64 bit) and counter = (step number (64 bit), slot, global replica index), so streams of
 * different (seed, replica) pairs never coincide -- seeds that differ by less than the replica
 * count do NOT alias.  The step number continues across calls on the same batch (the batch counts
 * the steps it has run), so repeated runs with one seed do not replay their draws; the molecule
 * of step s of a call is still s mod n_mol, as Loop() restarts its sweep (Ewald/main.jl:490).
 * Host-side proposals: one xoshiro256++ stream per chain seeded from a hash of (seed, global
 * replica index, steps already run). */

typedef struct {
    int64_t moves, launches;
    int64_t trans_attempt, trans_accept, rot_attempt, rot_accept, overlaps;
    double wall_ms;      /* host wall clock over the run */
    double kernel_ms;    /* sum of HIP-event durations of the move kernel (time_kernels); with more
                            than one stream launches overlap and a duration is the launch's span */
    double energy_sum;   /* sum over replicas of the running total energy at the end */
    int64_t timed_launches; /* launches that contributed to kernel_ms */
    int64_t torn_records;   /* result records that carried the launch stamp but failed their
                               checksum when first read (re-read until whole) */
    int64_t server_steps;   /* steps that ran on the persistent move server (option "persistent"):
                               `launches` then counts control-word posts, not kernel launches */
    int64_t device_decisions; /* moves whose accept decision the move kernel made itself (option
                               "accept_on_device"): the host did their bookkeeping only */
} mmc_run_stats;

/* An NPT chain of a one-replica batch: n_sweeps times { moves_per_sweep trial moves (mmc_batch_run:
 * Loop(), Ewald/main.jl:487-644), then ONE volume move } -- Ewald/volumeChange.jl:59-147:
 *   vol_new = vol_old + (rand() - 0.5) * vmax                         :59
 *   test = exp(-beta (P dV - N ln(vol_new / vol_old) / beta + dE))    :129-130
 *   accepted if rand() < test                                         :132
 * with beta = 1 / temperature (energies are in K, so the pressure is in K / A^3), kappa = alpha /
 * L_new (Ewald/main.jl:290-291) and dE from the full recompute at the new volume.  The host decides;
 * the two uniforms of a volume move are Philox draws of the chain's own stream (seed, replica0)
 * at the step count it has reached, slot MMC_SLOT_VOLUME.  A move to a box below 2 r_cut is
 * rejected outright.  energy: in/out, the running total of the replica. */
#define MMC_SLOT_VOLUME 0x40000000u /* Philox slot of a volume move's two uniforms */
typedef struct {
    double pressure;         /* K / A^3 */
    double vmax;             /* A^3: dV is uniform in +- vmax / 2 */
    double alpha;            /* kappa * L (5.6 in Ewald/main.jl:290) */
    int64_t n_sweeps;
    int64_t moves_per_sweep; /* 0 = one per molecule (Ewald/main.jl:490) */
} mmc_npt_params;
typedef struct {
    int64_t vol_attempt, vol_accept;
    double box;              /* at the end */
    double volume_sum;       /* sum over the sweeps of the volume after each volume move */
    double volume_ms;        /* host wall clock spent in the volume moves */
} mmc_npt_stats;
int32_t mmc_batch_run_npt(mmc_batch *b, const mmc_run_params *p, const mmc_npt_params *q,
                          double *energy, mmc_run_stats *stats, mmc_npt_stats *npt_stats);

/* ---- Per-replica boxes: independent NPT replicas in one batch ----------------------------------
 * mmc_batch_set_boxes switches a batch to per-replica mode: replica r lives in box boxes[r] with
 * kappa_r = alpha / boxes[r] (Ewald/main.jl:290-291), its own cfac row (PrepareEwaldVariables,
 * ewalds.jl:45-103, over the shared k-vector list) and its own erfc(kappa_r r)/r table.  The
 * coordinates are whatever mmc_batch_set_replica put there (the call does not rescale them); call
 * mmc_batch_recip_long afterwards, as after creation.  Every box must be at least 2 r_cut
 * (MMC_ERR_ARG).  The erfc table must cover the smallest box a volume move admits, L = 2 r_cut:
 * kappa = alpha / (2 r_cut) <= MMC_QQ_KAPPA_MAX and kappa * sqrt(r_cut^2 + 100) <= MMC_QQ_XMAX,
 * with identical 3-atom molecules; otherwise MMC_ERR_UNSUPPORTED and no state changes (SPC/E, 750
 * molecules, r_cut 10, alpha 5.6: 3.96 <= 4).  The call may be repeated; the mode is never left.
 * In per-replica mode:
 *   - mmc_batch_recip_long, mmc_batch_potential_ewald and mmc_batch_run use each replica's box.
 *     Trial moves are drawn on the device (option "device_moves" is set and cannot be cleared)
 *     and evaluated by kernel 1 (one workgroup per move); the host decides.  A replica in which
 *     an atom pair overlaps gets total energy +inf and n_overlap = 1 from potential_ewald.
 *   - these return MMC_ERR_UNSUPPORTED and compute nothing: mmc_batch_eval, mmc_batch_settle,
 *     mmc_batch_rdf, mmc_batch_qq_table, mmc_batch_run_chains, mmc_batch_run_npt,
 *     mmc_batch_volume_change, mmc_batch_volume_trial / _accept / _reject,
 *     mmc_batch_set_orientations, and mmc_batch_set_option for "kernel" 0, 2 or 4 (the wave and
 *     latency kernels), "persistent" = 1 (the move server) and "device_moves" = 0.
 * mmc_batch_get_boxes: every replica's box (the shared box when the mode is off). */
int32_t mmc_batch_set_boxes(mmc_batch *b, const double *boxes, double alpha);
int32_t mmc_batch_get_boxes(mmc_batch *b, double *boxes);
/* One batched volume trial (volumeChange.jl:59-111): new_boxes[r] == 0 leaves replica r where it
 * is.  Every replica's state is copied aside on the device; each replica that moves is rescaled
 * about the centres of mass (:62-80) and gets its cfac row and table for alpha / L_new; tot[r] is
 * the total energy of every replica at its (new) box.  Follow with mmc_batch_volume_settle:
 * accept[r] != 0 keeps a moved replica's new state at no cost; every other replica (rejected, or
 * not moved) gets back coordinates, S(k), tables and box bit for bit, in one launch. */
int32_t mmc_batch_volume_trial_replicas(mmc_batch *b, const double *new_boxes, mmc_totals *tot);
int32_t mmc_batch_volume_settle(mmc_batch *b, const int32_t *accept);
/* mmc_batch_run_npt's chain for every replica: n_sweeps x { a sweep of trial moves for all
 * replicas, then one volume move per replica, all replicas in one batched trial }.  Replica r's
 * two uniforms are Philox draws of its stream (seed, replica0 + r) at the step count reached, slot
 * MMC_SLOT_VOLUME; a box below 2 r_cut is rejected outright; the host decides.  pressures: [R]
 * K / A^3, or NULL for q->pressure everywhere.  q->alpha must be the alpha of mmc_batch_set_boxes.
 * energies: in/out [R] running totals.  per_replica: [R]; volume_ms is the wall clock of the
 * batched volume moves, the same for every replica. */
int32_t mmc_batch_run_npt_replicas(mmc_batch *b, const mmc_run_params *p, const mmc_npt_params *q,
                                   const double *pressures, double *energies, mmc_run_stats *stats,
                                   mmc_npt_stats *per_replica);

/* The driver's counter-based generator, exposed for known-answer tests and for callers that
 * want to re-derive a chain's draws: Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11). */
int32_t mmc_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);

/* energies: in/out running total energy per replica (R doubles), as `total.energy` (:599). */
int32_t mmc_batch_run(mmc_batch *b, const mmc_run_params *p, double *energies,
                      mmc_run_stats *stats);

/* Per-chain bookkeeping of Loop(): running totals, block-average accumulators and the two
 * step-size controllers.  One per replica; persists across mmc_batch_run_chains calls. */
typedef struct {
    double dr_max, dphi_max;       /* totProps.dr_max / totProps.dphi_max  (Ewald/main.jl:523,536) */
    double energy, virial;         /* total.energy, total.virial           (Ewald/main.jl:599-601) */
    double avg_energy, avg_virial; /* averages.energy / .virial: the running total added after
                                      EVERY trial move, accepted or not    (Ewald/main.jl:606-625) */
    int64_t steps_taken;           /* totProps.totalStepsTaken             (Ewald/main.jl:641) */
    int64_t overlaps;              /* ovr_count                            (Ewald/main.jl:595-597) */
    /* trans_moves / rot_moves :: Moves (Ewald/structs.jl), fields as used by Adjust! */
    int64_t trans_naccepp, trans_attempp, trans_naccept, trans_attempt;
    int64_t rot_naccepp, rot_attempp, rot_naccept, rot_attempt;
    double trans_set_value, rot_set_value; /* target acceptance ratios (Moves.set_value) */
} mmc_chain;

/* As mmc_batch_run, with every chain carrying its own step sizes and bookkeeping: p->dr_max and
 * p->dphi_max are ignored, chains[r].energy replaces energies[r].  After the trial move of the
 * last molecule of a sweep, Adjust!(trans_moves, box) and Adjust_rot!(rot_moves, box) run for the
 * chain exactly as at the end of Loop()'s inner loop (Ewald/main.jl:645-651, adjust.jl:1-83);
 * a controller that saw no attempt since its last call is left alone (the reference would divide
 * 0/0 there).  adjust = 0 keeps the step sizes fixed. */
int32_t mmc_batch_run_chains(mmc_batch *b, const mmc_run_params *p, mmc_chain *chains,
                             int32_t adjust, mmc_run_stats *stats);

/* The status line Loop() prints after every block (Ewald/main.jl:667-679), from one chain's record:
 *   "Block: %4d, Energy: %8.2f, Ratio trans: %4.2f, dr_max: %4.2f, Ratio rot: %4.2f, dphi_max: %4.2f,
 *    instant energy: %8.2f, overlap count: %4d, pressure: %8.2f"
 * with Energy = averages.energy / totalStepsTaken / n_mol, the two acceptance ratios
 * naccept / attempt, instant energy = total.energy / n_mol, and
 * pressure = ideal_term + total.virial / box^3: the reference hard-codes ideal_term = 4.60453
 * (main.jl:677); pass rho * T for auxillary.jl:121-123's Pressure(vir, rho, T, vol).  A ratio with
 * no attempt prints NaN, as Julia's 0/0 does.  Writes at most `len` bytes including the
 * terminator; returns MMC_ERR_ARG if the line does not fit. */
int32_t mmc_chain_block_line(const mmc_chain *chain, int64_t block, int64_t n_mol, double box,
                             double ideal_term, char *buf, int64_t len);

/* ---- Candidate lists of the move kernel's COM scan ---------------------------------------------
 * Where mmc_batch_run / mmc_batch_eval run the wave kernel with one part per move (large batches of
 * identical molecules, one box), a trial move tests only the chosen molecule's CANDIDATES -- the
 * molecules within gate + skin of it when the replica's lists were last built -- instead of every
 * centre of mass, while a per-replica bound on how far any molecule has moved since then proves that
 * no molecule outside the list can pass the prefilter; otherwise, and until stale lists have been
 * rebuilt, the step scans in full.  The neighbours the pair loops see are the same in the same order:
 * every result is bit for bit that of option "candidate_lists" = 0.
 * MEMORY: 2 * 256 bytes per molecule and replica (+ 8 per molecule), allocated when the batch first runs
 * that kernel: 23.9 GB for 61 440 replicas of 750 molecules.  If it does not fit with a sixteenth of the
 * device (at least 1 GiB) to spare, the batch runs without lists and mmc_batch_cand_stats says so.
 * Options (mmc_batch_set_option): "candidate_lists" 1 (default) / 0; "cand_skin", the skin in
 * THOUSANDTHS of an Angstrom (default 2000): smaller = shorter lists that are rebuilt sooner; lists of
 * more than 256 molecules are not used.
 * mmc_batch_cand_stats: out[0] steps that took a list, [1] steps of the same launches that scanned in
 * full, [2] rebuilds (replica x times), [3] bytes allocated, [4] launches of the rebuild kernel,
 * [5] state: 0 switched off, 1 in use, 2 not allocated (memory), 3 not applicable (mixed systems,
 * per-replica boxes, a skin too small for the gate), 4 not needed so far; [6] the budget and [7] the
 * lists' threshold in code units (mmc_cand_thresholds).  Counts are sums over the batch's life.
 * mmc_cand_thresholds / mmc_cand_within: the integer arithmetic of the per-step test, pure host
 * functions (no device): out[0] the prefilter's threshold for `gate` (A) in a box, out[1] the lists'
 * for gate + skin, out[2] the budget B; out[k] = 1 where sqrt(a2[k]) + sqrt(d2[k]) <= B is PROVEN on
 * the squares (it may say 0 where the sum is within rounding of B, never 1 where it exceeds it). */
int32_t mmc_batch_cand_stats(mmc_batch *b, int64_t *out /* [8] */);
int32_t mmc_cand_thresholds(double gate, double skin, double box, uint32_t *out /* [3] */);
int32_t mmc_cand_within(int64_t n, const uint32_t *a2, const uint32_t *d2, uint32_t budget, uint8_t *out /* [n] */);

/* ---- Parallel tempering: per-replica temperatures and ladder exchanges ---------------------------
 * mmc_batch_set_temperatures gives replica r its own temperature temps[r] (K): mmc_batch_run,
 * mmc_batch_run_chains and mmc_batch_run_npt_replicas then decide replica r's trial moves with
 * Metropolis(dU / temps[r]) on every path (host decisions and the move kernel's own), and
 * mmc_batch_run_npt_replicas uses beta_r = 1 / temps[r] in the volume criterion as well;
 * p->temperature is ignored but must still be > 0.  temps == NULL switches the array off again.
 * An array of R equal values is the scalar chain bit for bit: the decision is the same expression
 * dU / T with the same draws.  mmc_batch_run_npt (the one-replica chain) returns
 * MMC_ERR_UNSUPPORTED while temperatures are set.  MMC_ERR_ARG, no state changed: a value <= 0 or
 * not finite.  MMC_ERR_STATE: proposals outstanding (mmc_batch_settle) or a volume trial open.
 * The entry points that take their own `temperature` argument (mmc_batch_widom*,
 * mmc_batch_deletion, mmc_batch_volume_perturb) never read the batch's array.
 * mmc_batch_get_temperatures: the array as it stands (exchanges permute it), 0.0 everywhere when
 * off; it does not depend on any run's p->temperature. */
int32_t mmc_batch_set_temperatures(mmc_batch *b, const double *temps /* [R]; NULL = off */);
int32_t mmc_batch_get_temperatures(mmc_batch *b, double *temps /* [R]; run-independent: 0.0 when off */);

/* One round of ladder exchanges, decided on the host: a pure function of its arguments -- no
 * device, no batch.  A swap exchanges TEMPERATURES, not configurations: no replica state moves.
 * Layout: ladder l is replicas [l n_rungs, (l + 1) n_rungs); rung[r] in 0..n_rungs-1 is the rung
 * of its ladder that replica r holds now (a permutation within every ladder).  For every ladder l
 * and k = parity, parity + 2, ... with k + 1 < n_rungs:
 *   a = the replica of the ladder holding rung k, b = the one holding rung k + 1
 *   attempt[k]++
 *   D = (1 / temps[a] - 1 / temps[b]) * ((energies[a] - energies[b]) + pressure * (volumes[a] - volumes[b]))
 *       (volumes == NULL, NVT:  D = (1 / temps[a] - 1 / temps[b]) * (energies[a] - energies[b]))
 *   u = the first uniform of the Philox draw with key = seed, counter = (round (64 bit),
 *       MMC_SLOT_EXCHANGE, (uint32_t)(replica0 + l n_rungs + k)) -- "Random streams" above:
 *       ((x0 << 32 | x1) >> 11) * 2^-53 of the four output words x0..x3
 *   accepted if and only if energies[a], energies[b] and D are all finite and (D >= 0 or
 *       u < exp(D)) -- exp of the host's libm
 *   on acceptance: temps[a] <-> temps[b], rung[a] <-> rung[b], accept[k]++
 * A replica whose energy is +inf (an overlapping start: mmc_batch_potential_ewald's convention)
 * never swaps.  attempt / accept: [n_rungs - 1], accumulated over calls and ladders.
 * MMC_ERR_ARG, nothing changed: n_ladders < 1, n_rungs < 2, parity not 0 or 1, a NULL array other
 * than volumes, rung not a permutation of 0..n_rungs-1 within a ladder, a temperature that is not
 * positive and finite.
 * Sharding: a rank's share of a larger ensemble holds whole ladders, so its replica0 is a multiple
 * of n_rungs (sharding.shard / shard_total check it when given n_rungs). */
#define MMC_SLOT_EXCHANGE 0x60000000u /* Philox slot of a ladder exchange's uniform */
int32_t mmc_exchange_round(int64_t n_ladders, int32_t n_rungs, int32_t parity, uint64_t seed,
                           uint64_t replica0, uint64_t round, double pressure,
                           const double *energies, const double *volumes /* NULL: NVT */,
                           double *temps /* in/out */, int32_t *rung /* in/out */,
                           int64_t *attempt, int64_t *accept /* [n_rungs - 1], accumulated */);
/* mmc_exchange_round on the batch's own temperatures (R / n_rungs ladders), which are then uploaded
 * again.  With per-replica boxes the volumes are box^3 of mmc_batch_get_boxes; otherwise NVT, and
 * `pressure` is ignored.  MMC_ERR_STATE: no temperatures set, proposals outstanding or a volume
 * trial open.  MMC_ERR_ARG: R is not a multiple of n_rungs, and mmc_exchange_round's. */
int32_t mmc_batch_exchange(mmc_batch *b, int32_t n_rungs, int32_t parity, uint64_t seed, uint64_t replica0,
                           uint64_t round, double pressure, const double *energies, int32_t *rung,
                           int64_t *attempt, int64_t *accept);
/* n_rounds x { p->n_steps trial moves for every replica (mmc_batch_run), one exchange }: round i
 * uses round = round0 + i and parity = (round0 + i) & 1, with p->seed and p->replica0.  energies:
 * in/out [R] running totals (in Wolf style the Wolf totals).  stats: summed over the rounds as
 * mmc_batch_run_npt_replicas sums them.  One-box batches only (MMC_ERR_UNSUPPORTED with
 * per-replica boxes: drive an NPT ladder as mmc_batch_run_npt_replicas of one sweep followed by
 * mmc_batch_exchange).  Errors otherwise as mmc_batch_exchange and mmc_batch_run; the arguments of
 * the exchange are checked before the first move. */
int32_t mmc_batch_run_exchange(mmc_batch *b, const mmc_run_params *p, int64_t n_rounds, int32_t n_rungs,
                               uint64_t round0, double *energies, int32_t *rung,
                               int64_t *attempt, int64_t *accept, mmc_run_stats *stats);

/* ---- Widom test-particle insertion: the excess chemical potential of every replica ------------
 * The reference has no insertion code (its README names free energies and adsorption as goals);
 * the insertion energy is DEFINED through its own total energy, potential(..., "ewald")
 * (Ewald/energy.jl:946-1032): dU is what that total changes by when the test molecule is appended
 * as molecule N + 1 of the replica's current configuration,
 *   dU = d_lj + d_real + d_recip
 *   d_lj    = LJ_poly_dU(N+1)                       energy.jl:209-290 (COM gate, eps > 0.001)
 *   d_real  = EwaldShort(N+1)                       ewalds.jl:892-910 -> EwaldReal :293-376
 *             (slack r_cut^2 + 100; 0 when an atom pair overlaps, :359-360)
 *   d_recip = factor sum_k cfac_k (2 Re(conj(S_k) s_k) + |s_k|^2)  RecipLong(N+1) - RecipLong(N), :538-604
 *           - factor kappa / sqrt(pi) sum_a q_a^2   EwaldSelf(N+1) - EwaldSelf(N), :829-833
 * S_k: the replica's committed structure factor over the batch's half-space k list (doubled
 * weights) -- built by mmc_batch_recip_long (call it once after creation, as before the first
 * trial move) and kept by the moves since; s_k: the test molecule's own, by the reference's phase
 * recurrence.  Up to summation
 * order this is potential(N+1) - potential(N).
 *   - The test molecule is rigid with the atom types and charges of molecule 1; its atoms sit at
 *     COM + R offsets[a] (offsets [3][3], A, from the COM).
 *   - Overlap: an atom pair with r^2 < 0.5 and opposite charges (ewalds.jl:359).  An overlap, and
 *     a dU that is NaN or +-inf (an atom exactly on another: the LJ term is Inf - Inf), has weight
 *     0 and counts in n_overlap; ovl_out[i] bit 0 = overlap, bit 1 = non-finite dU.
 *   - Random insertions: Philox4x32-10, key = seed, counter = (draw0 + j, slot, replica index in
 *     the batch), slots MMC_SLOT_WIDOM + 0, 1, 2 (six uniforms u0..u5): COM = (u0, u1, u2) L, in
 *     [0, L) (boundaries.jl:16-26); orientation Shoemake's uniform unit quaternion of (u3, u4, u5),
 *     q = (w, x, y, z) = (sqrt(u3) cos 2 pi u5, sqrt(1-u3) sin 2 pi u4, sqrt(1-u3) cos 2 pi u4,
 *     sqrt(u3) sin 2 pi u5), as its rotation matrix.
 *   - boltz_sum[r] += exp(-dU / T) (T in K, like the energies) over the call's insertions, added in
 *     insertion order: the result is bit-identical whatever the grid or option "wave_wgs";
 *     n_overlap[r] += the insertions of weight 0.  Call once per sweep to accumulate.
 *   - mol_out: [R][n_insert][12] atoms (9) then COM (3) of each insertion; du_out: [R][n_insert][3]
 *     (d_lj, d_real, d_recip); ovl_out: [R][n_insert].  Each may be NULL.
 *   - Read-only: coordinates, S(k), the chains' flags, step counters and random streams are not
 *     touched; a chain run with these calls interleaved is bit-identical to one without.
 * Preconditions as mmc_batch_potential_ewald: no proposals outstanding (MMC_ERR_STATE), no volume
 * trial in flight (MMC_ERR_STATE).  MMC_ERR_UNSUPPORTED, nothing computed: per-replica boxes
 * (mmc_batch_set_boxes), or a system the table kernels do not take (not identical 3-atom molecules,
 * or a cutoff / kappa outside the erfc table).  MMC_ERR_ARG: n_insert < 1, a NULL required array,
 * temperature <= 0 or not finite, non-finite offsets or molecules.
 * mmc_batch_widom_at evaluates the caller's molecules mol_in [R][n_insert][12] (same layout as
 * mol_out) with the same kernel. */
#define MMC_SLOT_WIDOM 0x50000000u /* Philox slots of an insertion: +0..+5 (+3, +4, +5: B of mmc_batch_widom_pair) */
/* (`temperature` is this call's own argument: the batch's per-replica temperatures,
 * mmc_batch_set_temperatures, are not read) */
int32_t mmc_batch_widom(mmc_batch *b, int64_t n_insert, uint64_t seed, int64_t draw0,
                        const double *offsets, double temperature, double *boltz_sum,
                        int64_t *n_overlap, double *mol_out, double *du_out, uint8_t *ovl_out);
/* (`temperature` is this call's own argument: the batch's per-replica temperatures,
 * mmc_batch_set_temperatures, are not read) */
int32_t mmc_batch_widom_at(mmc_batch *b, int64_t n_insert, const double *mol_in, double temperature,
                           double *boltz_sum, int64_t *n_overlap, double *du_out, uint8_t *ovl_out);

/* ---- Foreign solutes: hydration free energies (Henry constants) of every replica ----------------
 * mmc_batch_widom inserts a copy of the batch's own molecule; these calls insert a rigid solute
 * that is NOT water -- methane, an ion, an alcohol -- as a test particle: the excess chemical
 * potential at infinite dilution.  The insertion energy is defined exactly as mmc_batch_widom's,
 * through the reference's potential(..., "ewald") (Ewald/energy.jl:946-1032): dU is what that
 * total changes by when the solute is appended as molecule N + 1 with its own atom types,
 *   d_lj    = LJ_poly_dU(N+1)        energy.jl:209-290: waters whose COM lies within lj_rcut of the
 *             solute's reference point c (vector1D per axis, strict <); over those all S x 3 atom
 *             pairs on the per-pair vector1D image; a pair counts when r^2 < r_cut^2 + 100 and
 *             eps > 0.001; the sum times 4
 *   d_real  = EwaldShort(N+1)        ewalds.jl:892-910 -> :293-376: COM gate on qq_rcut; a pair with
 *             r^2 < 0.5 and q_a q_b < 0 is an overlap (d_real = 0, flag bit 0); else factor times
 *             sum q_a q_b erfc(kappa r) / r over pairs with r^2 < r_cut^2 + 100 (the batch's table)
 *   d_recip = factor sum_k cfac_k (2 Re(conj(S_k) s_k) + |s_k|^2) - factor kappa / sqrt(pi) sum_a q_a^2
 *             s_k = sum_a q_a exp(2 pi i k . r_a / L) by the reference's phase recurrence, over the
 *             batch's half-space k list against the replica's committed S(k); computed whether or
 *             not the insertion overlaps.
 * The solute: n_sites = S sites, 1 <= S <= MMC_SOLUTE_MAX_SITES;
 *   - offsets [S][3] (A) from its reference point c.  c is the "centre of mass" of the reference's
 *     molecule-level gates and the caller's choice (io.solute_from_decks takes the mass COM);
 *   - charge [S];
 *   - eps [S][3], sig [S][3] (K, A) against the three atom slots of the batch's molecule, already
 *     mixed: the entries eps_ij[type_a, type_slot] of the reference's Tables.
 *   - A solute whose charges are all zero has d_real = d_recip = +0.0 exactly and S(k) is not read.
 *   - A net-charged solute is allowed.  NO neutralising-background term is added, because the
 *     reference's total energy has none: d_recip of an ion is the bare expression above.
 *   - The constant intramolecular Ewald term of the solute is absent, as in mmc_batch_widom
 *     (observables.ewald_intra_energy takes any number of sites).
 * Draws: those of mmc_batch_widom -- the same three Philox slots MMC_SLOT_WIDOM + 0, 1, 2 with
 * counter draw0 + j: c = (u0, u1, u2) L, Shoemake's rotation Rm of (u3, u4, u5), site a at
 * c + Rm offsets[a].  For one (seed, draw0) the reference points are bit for bit the COMs
 * mmc_batch_widom draws and the probes of mmc_batch_cavity (observables.solute_molecules).
 * mol_out (mmc_batch_widom_solute) / mol_in (_at): [R][n_insert][S + 1][3], the sites, then c.
 * du_out [R][n_insert][3] (d_lj, d_real, d_recip); ovl_out [R][n_insert], bit 0 = overlap, bit 1 =
 * non-finite dU.  boltz_sum[r] += exp(-dU / T) in insertion order and n_overlap[r] += the
 * insertions of weight 0, exactly as mmc_batch_widom: bit-identical whatever the grid or option
 * "wave_wgs".  mol_out, du_out and ovl_out may be NULL.  Read-only for the chains.
 * MMC_ERR_ARG (in this order; what needs no batch is refused without one): n_sites outside
 * 1..MMC_SOLUTE_MAX_SITES, a NULL required array, n_insert < 1, temperature <= 0 or not finite,
 * a non-finite charge, eps, sig, offset or coordinate, eps < 0 or sig < 0, replicas x n_insert above
 * 2^31 - 1.  MMC_ERR_STATE and MMC_ERR_UNSUPPORTED as mmc_batch_widom (proposals outstanding, S(k)
 * stale; per-replica boxes, Wolf style, a system the table kernels do not take).  Nothing is
 * written on a refusal. */
#define MMC_SOLUTE_MAX_SITES 16
/* (`temperature` is this call's own argument: the batch's per-replica temperatures,
 * mmc_batch_set_temperatures, are not read) */
int32_t mmc_batch_widom_solute(mmc_batch *b, int32_t n_sites, const double *offsets, const double *charge,
                               const double *eps, const double *sig, int64_t n_insert, uint64_t seed,
                               int64_t draw0, double temperature, double *boltz_sum, int64_t *n_overlap,
                               double *mol_out, double *du_out, uint8_t *ovl_out);
/* (`temperature` is this call's own argument: the batch's per-replica temperatures,
 * mmc_batch_set_temperatures, are not read) */
int32_t mmc_batch_widom_solute_at(mmc_batch *b, int32_t n_sites, const double *charge, const double *eps,
                                  const double *sig, int64_t n_insert, const double *mol_in,
                                  double temperature, double *boltz_sum, int64_t *n_overlap,
                                  double *du_out, uint8_t *ovl_out);

/* ---- A fixed solute: chains around a solute, hydration shells of every replica --------------------
 * The calls above insert a solute as a test particle; no chain feels it.  mmc_batch_set_solute holds
 * ONE rigid solute of 1..MMC_SOLUTE_MAX_SITES sites fixed at the same place in every replica: from
 * then on every trial move (mmc_batch_eval, mmc_batch_run, _run_chains, _run_exchange), every total
 * (mmc_batch_recip_long, mmc_batch_potential_ewald) and the saved state see it as molecule N + 1 of
 * the reference's potential(..., "ewald").  A solute that is held fixed is all one solute needs, by
 * translation invariance; it is never moved and needs no commit.  Definitions, gates, the overlap rule,
 * "no neutralising background" and "no intramolecular term" are those stated for
 * mmc_batch_widom_solute: per trial move of a water the solute adds LJ_poly_dU's and EwaldReal's terms
 * of that water against the S sites (COM gate on the solute's reference point c, per-pair vector1D,
 * r^2 < r_cut^2 + 100, eps > 0.001, the batch's erfc table, overlap = r^2 < 0.5 and q_a q_b < 0), and
 * S(k) carries the constant S_sol(k) = sum_a q_a exp(2 pi i k . r_a / L).  Nothing changes while no
 * solute is set.
 *   mmc_batch_set_solute(b, n_sites, mol, charge, eps, sig)
 *     mol [S + 1][3]: the sites, then the reference point c, as mol_in of mmc_batch_widom_solute_at;
 *     charge [S]; eps, sig [S][3] against the three atom slots of the batch's molecule.  n_sites == 0
 *     removes the solute (the arrays are not read).  MMC_ERR_ARG, in mmc_batch_widom_solute_at's order
 *     and without a batch: n_sites outside 0..MMC_SOLUTE_MAX_SITES, a NULL array, a non-finite charge,
 *     eps or sig, eps < 0 or sig < 0, a non-finite coordinate.  MMC_ERR_STATE while proposals or a
 *     volume trial are outstanding.  MMC_ERR_UNSUPPORTED, with nothing changed, on a batch with
 *     per-replica boxes or in Wolf style and on a system the table kernels do not take.  If the new or
 *     the previous solute carries a charge, S(k) is stale until mmc_batch_recip_long (or
 *     mmc_batch_potential_ewald) -- the flag of the change from Wolf to Ewald style, and MMC_ERR_STATE
 *     from the same calls until then.  An uncharged solute neither reads nor stales S(k).
 *   mmc_batch_get_solute: *n_sites and the arrays as they were set; every pointer may be NULL.
 *   With a solute set
 *     - the host decides every move from the move kernel's records and one more, k_solute_move's, a
 *       launch per step: options "accept_on_device", "steps_per_launch" and "whole_call" fall back
 *       silently as they do wherever they do not apply, and mmc_run_stats::device_decisions is 0.
 *       Candidate lists, host or device proposals, parts, per-replica temperatures, chains with their
 *       virial (the solute's part included) and option "trace_steps" work as without one.  An explicit
 *       option persistent = 1 or kernel = 4 is MMC_ERR_UNSUPPORTED from the run (kernel = 4 from
 *       mmc_batch_eval too, which never takes the move server); chosen by size, the move server is
 *       not taken.
 *     - mmc_batch_recip_long adds S_sol(k) to both buffers before the energy is formed;
 *       mmc_batch_get_replica and the state record then carry S(k) of the N + 1 system.
 *     - mmc_batch_potential_ewald returns every field of mmc_totals as potential() of the N + 1 system:
 *       each water-solute pair twice in the halved double-counted sums, EwaldSelf over the solute's
 *       charges too.  A replica in which the solute overlaps a water has energy +inf and n_overlap
 *       one higher, as a replica with per-replica boxes reports an overlap.
 *     - MMC_ERR_UNSUPPORTED, nothing computed or changed (the energies would be another system's):
 *       mmc_batch_set_boxes, mmc_batch_set_coulomb_style(Wolf), mmc_batch_potential_wolf,
 *       mmc_batch_volume_change / _trial / _accept / _reject, mmc_batch_run_npt (and _npt_replicas,
 *       which needs the boxes), mmc_batch_widom*, mmc_batch_deletion, mmc_batch_forces,
 *       mmc_batch_volume_perturb, mmc_batch_pair_energy.  The observables that read coordinates only
 *       stay open and see the water.
 *   mmc_batch_solute_energy: u_lj[r], u_real[r] = the water-solute pair energy of replica r -- d_lj
 *     and d_real of mmc_batch_widom_solute_at at the solute's place, the summand of <u_sw> -- and
 *     ovl[r] = 1 where a pair overlaps (u_real = 0 then).  Lane l of the replica's wave adds the
 *     waters l, l + 64, ... in that order, the sites in order, and the 64 lane sums are added in a
 *     fixed order: bitwise independent of the launch.  MMC_ERR_STATE without a solute.  Read-only.
 *   mmc_batch_rdf_solute: uint64 counts hist[1 + S][3][numbins] (per_replica == 0, summed over the
 *     replicas) or hist[R][1 + S][3][numbins]: row 0 measured from c, row 1 + a from site a, each
 *     against the three water slots.  d = (the solute's point) - (the water's site); image, r, bin =
 *     ceil(r / dr), dr and the r_max rule exactly mmc_batch_rdf_sites'; a distance with 1 <= bin <=
 *     numbins is counted at [bin - 1] (a site exactly on the point is not counted).  hist is
 *     overwritten.  Arguments and preconditions as mmc_batch_rdf_sites; MMC_ERR_STATE without a
 *     solute.  Read-only.
 *   mmc_batch_hydration_map: the solute-centred maps, the first-order terms of grid inhomogeneous
 *     solvation theory.  The solute is fixed and the same in every replica, so the laboratory frame is
 *     its frame and one grid takes the waters of all replicas; nothing is aligned.  int64 maps
 *     [n_ch][cells + 2] (per_replica == 0, summed over the replicas) or [R][n_ch][cells + 2], n_ch =
 *     popcount(channel_mask), the channels in rising bit order, cells = (2 n_half)^3.  maps is
 *     overwritten, not accumulated, and untouched on any error.  Everything below is unfused fp64 in the
 *     order written, with IEEE sqrt and divide, dot(a,b) = (a.x b.x + a.y b.y) + a.z b.z
 *     (tests/hydration_map_ref.py restates it).
 *     Grid: a cube on the laboratory axes centred on the solute's reference point c (mol[S]).  Edges
 *       e_k = (double)k * cell, k = -n_half .. n_half; a coordinate p lies in cell k when
 *       e_k <= p < e_k+1, stored at index k + n_half; flat index (ix g + iy) g + iz with g = 2 n_half:
 *       mmc_batch_sdf's cell rule without folding.  A deposit with any coordinate in no cell is
 *       `outside`; a NaN counts as outside.
 *     Position of a water site w: x = w - c per component (water minus solute), then the image of
 *       mmc_batch_rdf_solute with the batch's box L: |x| > L / 2 (strict) moves x by one box.
 *     Channels.  Bits 0, 1, 2 (counts): every water deposits 1 at the cell of its slot-a site, a = 0, 1,
 *       2, each site with its own image.  Bits 3, 4, 5 (orientation): every water deposits Q30(e_z.x),
 *       Q30(e_z.y), Q30(e_z.z) at the cell of its slot-0 site; e_z is the unit bisector exactly as
 *       mmc_batch_sdf defines it: o_a = vector1D(s0, s_a), b = o1 + o2, nb2 = dot(b,b), e_z = b /
 *       sqrt(nb2); Q30(v) = v * 2^30 rounded to nearest, ties to even.  A water with nb2 zero or not
 *       finite has no frame: it deposits nothing and is counted in the channel's last slot.  Bit 6 is
 *       Q20(u_lj), bit 7 Q20(u_real), Q20(u) = u * 2^20 rounded likewise, deposited at the cell of the
 *       slot-0 site: the water's own pair energy with the solute in K by the definitions above (the COM
 *       gates on c, the slack cutoffs, eps > 0.001, the batch's erfc table), a fresh accumulator per
 *       water over the sites 0 .. S - 1 in order, u_lj = (0.0 + sum_lj) * 4 and u_real = factor * (0.0 +
 *       sum_qq): the summands of mmc_batch_solute_energy.  A water is `flagged` if it overlaps the
 *       solute, if u_lj or u_real is not finite, or if either has magnitude >= 2^20 K; a flagged water
 *       deposits into neither energy channel and is counted in the last slot of both.  With an
 *       uncharged solute u_real = 0 for every water and the erfc table is not read.
 *     Tail slots of every channel: slot `cells` holds the same quantity summed over the deposits that
 *       fell outside the cube; slot cells + 1 the number of waters left out (no frame for channels 3-5,
 *       flagged for 6-7, always 0 for 0-2).  So per replica a count channel sums to N exactly.  All sums
 *       are 64-bit integers added modulo 2^64: the result does not depend on the grid of the launch,
 *       on option "wave_wgs", on which channels are requested together or on the order of atomics.
 *     Checks, in this order.  MMC_ERR_ARG without looking at the batch: NULL maps; n_half < 1; cell not
 *       finite or <= 0; channel_mask outside 1..255; (2 n_half)^3 > MMC_HMAP_MAX_CELLS (n_half <= 12).
 *       Then the batch (NULL: MMC_ERR_ARG); MMC_ERR_STATE while proposals or a volume trial are
 *       outstanding; MMC_ERR_STATE without a solute; MMC_ERR_ARG when (double)n_half * cell > L / 2 (the
 *       cube would reach a second image).  Read-only: S(k), the streams and mmc_state_info are not
 *       touched.  The per-replica output is one device allocation of R n_ch (cells + 2) words; a
 *       device that cannot make it fails the call with the allocation's status (the call is not cut
 *       into chunks of replicas).
 *     observables.hydration_density, _polarisation, _energy, _radial_average turn the maps into g(x, y,
 *     z), <e_z>, the mean u_sw per water and per volume, and shell averages. */
#define MMC_HMAP_CHANNELS 8
#define MMC_HMAP_MAX_CELLS 16384      /* 64-bit cells in 128 KB of a workgroup's LDS */
#define MMC_HMAP_VEC_SCALE 1073741824.0 /* 2^30 */
#define MMC_HMAP_E_SCALE   1048576.0    /* 2^20, = MMC_PAIRE_SCALE */
int32_t mmc_batch_set_solute(mmc_batch *b, int32_t n_sites, const double *mol, const double *charge,
                             const double *eps, const double *sig);
int32_t mmc_batch_get_solute(mmc_batch *b, int32_t *n_sites, double *mol, double *charge, double *eps,
                             double *sig);
int32_t mmc_batch_solute_energy(mmc_batch *b, double *u_lj, double *u_real, uint8_t *ovl);
int32_t mmc_batch_rdf_solute(mmc_batch *b, int32_t numbins, double r_max, int32_t per_replica,
                             uint64_t *hist);
int32_t mmc_batch_hydration_map(mmc_batch *b, int32_t n_half, double cell, int32_t channel_mask,
                                int32_t per_replica, int64_t *maps);

/* ---- A fixed solute: the mean force, field and potential on it ---------------------------------------
 * What the water does to the solute of mmc_batch_set_solute, in every replica, in one read-only pass
 * over the coordinates and the committed S(k): the solvent's force and torque on the held solute (the
 * integrand of a potential of mean force by constrained integration), the electrostatic potential at
 * its sites (dU/dq_a, the integrand of a charging free energy) and the electric field there.  The
 * reference has no forces; as for mmc_batch_forces they are DEFINED as gradients of its own total.  The
 * differenced energy U is every term of potential(..., "ewald") (energy.jl:946-1032) of the N + 1 system
 * that depends on the solute, each pair once, with the reference point c and all COMs frozen:
 *   U = LJ_poly_dU(N + 1) (energy.jl:209-290) + EwaldShort(N + 1) (ewalds.jl:892-906, EwaldReal :293-376)
 *       + factor RecipLong(all N + 1 molecules) (ewalds.jl:538-602) + EwaldSelf(the solute's charges)
 *       (ewalds.jl:829-833),
 * at fixed neighbour sets: the COM gates and the atom slack decide which pairs count and are not
 * differentiated.  Site a is at r_a with charge q_a.  A water j is gated by its COM against c exactly as
 * in the moves: rij = vector1D(com_j, c), |rij|^2 < r_cut^2 (strict; energy.jl:248-254 for LJ,
 * ewalds.jl:334-340 for qq); the qq gate is applied WHETHER OR NOT the solute is charged, because phi
 * and the field of an uncharged site are outputs too.  For water atom b: rab = vector1D(atom b, site a)
 * (site minus atom, one box moved where |.| >= L / 2), u = (rab.x^2 + rab.y^2) + rab.z^2 unfused.
 *   Lennard-Jones site force (LJ gate, u < lj_rcut^2 + 100, eps_ab > 0.001; energy.jl:270-281), with
 *   s2 = sig_ab^2 / u, s6 = s2^3, s12 = s6^2:
 *     site_lj[a] += 24 eps_ab (2 s12 - s6) / u * rab
 *   Real-space field and potential (qq gate, u < qq_rcut^2 + 100; ewalds.jl:359-367), r = sqrt(u):
 *     field[a] += factor q_b (erfc(kappa r) / r + 2 kappa / sqrt(pi) exp(-kappa^2 u)) / u * rab
 *     phi[a]   += factor q_b erfc(kappa r) / r
 *   erfc(kappa r) / r from the batch's table where it covers u (u >= 0.25), from the series below it.
 *   Reciprocal part, over the batch's half-space list with weights cfac_k and integer vectors n_k, the
 *   replica's committed S_k (it includes the solute's constant S_sol) and e_{a,k} = exp(2 pi i n_k . r_a
 *   / L) by the reference's phase recurrence (ewalds.jl:564-585):
 *     field[a] += factor (4 pi / L) sum_k cfac_k n_k Im(conj(S_k) e_{a,k})
 *     phi[a]   += 2 factor sum_k cfac_k Re(conj(S_k) e_{a,k})
 *     phi[a]   -= 2 factor kappa / sqrt(pi) q_a                        (EwaldSelf)
 *   So phi[a] = dU/dq_a exactly (U is quadratic in the charges; the term of S_sol against itself holds
 *   the solute's own periodic images and its intramolecular reciprocal part, as U does), and the site
 *   force is f_a = site_lj[a] + q_a field[a] = -dU/dr_a.  recip_out[r][a] = the three reciprocal field
 *   components and the reciprocal potential (without the self term) alone.
 *   Per replica, with d_a = vector1D(c, r_a) as mmc_batch_forces:
 *     F = sum_a f_a,  tau = sum_a d_a x f_a   (sites in index order, from zero)
 *   No intramolecular term, as everywhere for a solute: for a two-body "solute" the caller adds the
 *   direct interaction of its two parts.
 * Units: K / A (forces), K (torque), K / (e A) (field), K / e (phi).
 * flags_out[r]: bit 0 (MMC_WIDOM_OVERLAP's value 1) a site and a water atom of opposite charges with
 *   u < 0.5 inside the qq gate (the moves' rule, ewalds.jl:359); bit 1 (value 2) some output not finite
 *   (an atom exactly on a site).  A flagged replica has zeros in every row.
 * Order of summation: for each site, lane l of the replica's wave adds the waters l, l + 64, ... in that
 *   order, atoms b = 0, 1, 2, then the k-vectors l, l + 64, ...; the 64 lane sums are added in a fixed
 *   order.  No grid, option "wave_wgs", shard or set of requested outputs changes a bit.
 * Every output may be NULL; those given are overwritten: force_out, torque_out [R][3]; site_lj_out,
 *   field_out [R][S][3]; phi_out [R][S]; recip_out [R][S][4]; flags_out [R].
 * Read-only: coordinates, S(k), streams and counters are untouched.  On any error every output is
 *   untouched.  MMC_ERR_ARG: every output NULL (without looking at the batch), a NULL batch.
 *   MMC_ERR_STATE: proposals or a volume trial outstanding, no solute set, a run that failed half-way,
 *   S(k) stale (a charged solute set or removed before mmc_batch_recip_long; an uncharged solute does
 *   not stale S(k) and the call works).  tests/solute_force_ref.py restates every output. */
int32_t mmc_batch_solute_forces(mmc_batch *b, double *force_out, double *torque_out, double *site_lj_out,
                                double *field_out, double *phi_out, double *recip_out, uint8_t *flags_out);

/* ---- Solute pairs: potentials of mean force at infinite dilution ------------------------------------
 * How two foreign solutes A and B interact through the solvent -- the methane-methane contact and
 * solvent-separated minima, an ion pair -- from test particles (potential distribution theorem):
 *   g_AB(d) = < exp(-dU_AB(d) / T) >_N / ( < exp(-dU_A / T) >_N < exp(-dU_B / T) >_N ),  w(d) = -T ln g_AB(d)
 * dU_AB(d) is what the reference's potential(..., "ewald") (Ewald/energy.jl:946-1032) changes by when
 * A and B are appended d apart as molecules N + 1 and N + 2.  One call evaluates, per insertion, A
 * and B at n_sep = K separations along one random ray: the three averages for all K in one pass.
 * The solutes: A of n_sites_a = S_A sites, B of S_B, each described as mmc_batch_widom_solute
 * describes a solute (offsets [S][3] from a reference point, charge [S], eps / sig [S][3] against the
 * water's three slots), plus the A-B table eps_ab, sig_ab [S_A][S_B], already mixed.
 * S_A >= 1, S_B >= 1, S_A + S_B <= MMC_SOLUTE_MAX_SITES.  d [K], 1 <= K <= MMC_PAIR_MAX_SEP, each
 * finite, > 0 and < L / 2.
 * Draws: insertion j of replica r draws A exactly as mmc_batch_widom_solute (slots MMC_SLOT_WIDOM +
 * 0, 1, 2): mol_a_out is bit for bit its mol_out for the same (seed, draw0).  Slot +3 (u, v) gives
 * the ray's direction n = (s cos phi, s sin phi, z), z = 1 - 2 u, s = sqrt(1 - z^2), phi = 2 pi v;
 * slots +4 (u1, u2) and +5 (u3, its first uniform) give Shoemake's rotation R_B in the expressions
 * of mmc_batch_widom.  n and R_B serve all K separations of the insertion: c_B,k = c_A + d_k n,
 * wrapped per axis by the reference's rule (boundaries.jl:16-26: > L -> - L, < 0 -> + L); site b of B
 * at c_B,k + R_B off_b.
 * Terms, three rows of (lj, real, recip) per insertion and separation:
 *   dA    mmc_batch_widom_solute's definition for A against the N waters (the same for every k)
 *   dB_k  the same for B at placement k
 *   x_k   the A-B interaction as the reference computes it between molecules N + 1 and N + 2:
 *     x_lj    LJ_poly_dU restricted to the other solute (energy.jl:209-290): COM gate on
 *             vector1D(c_A, c_B) against lj_rcut, the per-pair vector1D image, a pair counts when
 *             r^2 < r_cut^2 + 100 and eps_ab > 0.001, the sum times 4
 *     x_real  EwaldShort restricted likewise (ewalds.jl:892-910 -> :293-376): gate on qq_rcut, the
 *             batch's erfc table, times factor; a site pair with r^2 < 0.5 and q_a q_b < 0 is an A-B
 *             overlap: x_real = 0 and flag bit 2
 *     x_recip factor sum_k cfac_k 2 Re(conj(s^A_k) s^B_k) on the batch's half-space k list
 *             (RecipLong(N+2) - RecipLong(N) minus the two single terms, ewalds.jl:538-604)
 * dU_AB,k = (dU_A + dU_B,k) + x_k, each dU and x_k formed as (lj + real) + recip.  No neutralising
 * background and no intramolecular term, as for foreign solutes: an ion pair's PMF therefore
 * INCLUDES the interaction with its periodic images.  With both solutes uncharged every real and
 * recip entry is exactly +0.0 and S(k) is not read.
 * flags [R][n_insert][1 + K]: entry 0 is A's (bit 0 overlap with a water, bit 1 dU_A non-finite);
 * entry 1 + k: bit 0 = B_k overlaps a water, bit 1 = dU_B,k non-finite, bit 2 = A-B overlap, bit 3 =
 * dU_AB,k non-finite.
 * Sums, all += in insertion order, bit-identical whatever the grid or option "wave_wgs":
 *   boltz_a [R], n_zero_a [R]        as mmc_batch_widom_solute's for A
 *   boltz_b [R][K], n_zero_b [R][K]  the single-solute sums of B at each placement (bits 0, 1)
 *   boltz_ab [R][K]                  sum exp(-dU_AB,k / T); weight 0, and counted in n_zero_ab
 *                                    [R][K], when any flag of A or of entry 1 + k is set.
 * Optional outputs (may be NULL): mol_a_out [R][n_insert][S_A + 1][3], mol_b_out
 * [R][n_insert][K][S_B + 1][3] (sites, then the reference point), du_out [R][n_insert][1 + 2 K][3]
 * (A, then B_0 .. B_K-1, then x_0 .. x_K-1), flags_out.  mmc_batch_widom_pair_at evaluates the
 * caller's mol_a_in and mol_b_in in those layouts with the same kernel; it takes no d.
 * Read-only for the chains.  MMC_ERR_ARG (in this order; what needs no batch is refused without
 * one): a site count outside 1..15 or their sum above MMC_SOLUTE_MAX_SITES, n_sep outside
 * 1..MMC_PAIR_MAX_SEP, a NULL required array (all six sums are required), n_insert < 1, temperature
 * <= 0 or not finite, a non-finite charge, eps, sig or offset, a negative eps or sig (eps_ab, sig_ab
 * included), d non-finite or <= 0; then with the batch: d >= L / 2, replicas x n_insert x (1 + K)
 * above 2^31 - 1, a non-finite coordinate.  MMC_ERR_STATE and MMC_ERR_UNSUPPORTED as
 * mmc_batch_widom_solute (proposals outstanding, S(k) stale; per-replica boxes, Wolf style, a
 * system the table kernels do not take).  Nothing is written on a refusal. */
#define MMC_PAIR_MAX_SEP 32
/* (`temperature` is this call's own argument: the batch's per-replica temperatures,
 * mmc_batch_set_temperatures, are not read) */
int32_t mmc_batch_widom_pair(mmc_batch *b, int32_t n_sites_a, const double *offsets_a, const double *charge_a,
                             const double *eps_a, const double *sig_a, int32_t n_sites_b, const double *offsets_b,
                             const double *charge_b, const double *eps_b, const double *sig_b, const double *eps_ab,
                             const double *sig_ab, int32_t n_sep, const double *d, int64_t n_insert, uint64_t seed,
                             int64_t draw0, double temperature, double *boltz_a, int64_t *n_zero_a, double *boltz_b,
                             int64_t *n_zero_b, double *boltz_ab, int64_t *n_zero_ab, double *mol_a_out,
                             double *mol_b_out, double *du_out, uint8_t *flags_out);
/* (`temperature` is this call's own argument: the batch's per-replica temperatures,
 * mmc_batch_set_temperatures, are not read) */
int32_t mmc_batch_widom_pair_at(mmc_batch *b, int32_t n_sites_a, const double *charge_a, const double *eps_a,
                                const double *sig_a, int32_t n_sites_b, const double *charge_b, const double *eps_b,
                                const double *sig_b, const double *eps_ab, const double *sig_ab, int32_t n_sep,
                                int64_t n_insert, const double *mol_a_in, const double *mol_b_in, double temperature,
                                double *boltz_a, int64_t *n_zero_a, double *boltz_b, int64_t *n_zero_b,
                                double *boltz_ab, int64_t *n_zero_ab, double *du_out, uint8_t *flags_out);

/* ---- Deletion energies: binding-energy histograms and the deletion half of BAR ------------------
 * The mirror image of mmc_batch_widom: the energy each EXISTING molecule is bound with.  The
 * reference has no deletion code; the deletion energy of molecule i of a replica's committed
 * configuration is DEFINED through its own total energy, potential(..., "ewald")
 * (Ewald/energy.jl:946-1032), as what that total loses when the molecule is taken out,
 *   dU = (d_lj + d_real) + d_recip
 *   d_lj    = LJ_poly_dU(i)                         energy.jl:209-290 (COM gate, eps > 0.001)
 *   d_real  = EwaldShort(i)                         ewalds.jl:892-910 -> EwaldReal :293-376, the
 *             factor applied (:905); 0, and the overlap flag set, when an atom pair of opposite
 *             charges has r^2 < 0.5 (:359-360)
 *   d_recip = factor sum_k cfac_k (2 Re(conj(S_k) s_k) - |s_k|^2)
 *           - factor kappa / sqrt(pi) sum_a q_a^2
 *             == RecipLong(N) - RecipLong(N \ i) (:538-604) + EwaldSelf(N) - EwaldSelf(N \ i) (:829-833)
 * S_k: the replica's committed structure factor over the batch's half-space k list (doubled
 * weights), molecule i included -- built by mmc_batch_recip_long and kept by the moves since, as
 * for mmc_batch_widom; s_k: molecule i's own, by the reference's phase recurrence.  Without
 * overlaps this is potential(N) - potential(N \ i) up to summation order, and term by term it is
 * what mmc_batch_widom_at returns for molecule i's coordinates inserted into the N - 1 others.  The
 * constant intramolecular Ewald term is absent, as in mmc_batch_widom
 * (observables.ewald_intra_energy).
 *   - Selection: sel [n_sel] 0-based molecules, the same for every replica; duplicates are allowed
 *     and evaluated twice.  sel == NULL: all N molecules in index order (n_sel is ignored).  Below,
 *     n = n_sel, or N when sel is NULL.
 *   - Flags (ovl_out [R][n]): bit 0 = overlap, bit 1 = dU is NaN or +-inf (an atom exactly on
 *     another) -- mmc_batch_widom's bits.  A flagged molecule enters no bin, no esum and no
 *     boltz_sum; it counts in n_flagged[r] (+=).
 *   - Histogram of dU over [u_lo, u_hi) in n_bins bins plus two outer counters: with
 *     s = n_bins / (u_hi - u_lo) in fp64 and k = floor((dU - u_lo) * s), unfused, dU < u_lo goes to
 *     slot 0, dU >= u_hi or k >= n_bins to slot n_bins + 1, everything else to slot k + 1.
 *     per_replica == 0: hist [n_bins + 2], summed over the replicas; else hist [R][n_bins + 2].
 *     Overwritten.  64-bit integer counts, exact and independent of the launch
 *     (observables.energy_bins is the same rule in numpy, for mmc_batch_widom's du_out).
 *   - esum [R][4], overwritten: the sums of d_lj, d_real and d_recip over the replica's unflagged
 *     selected molecules and their number (as a double).  boltz_sum[r] += sum exp(+dU / T), the
 *     inverse-Widom sum (T in K, like the energies).  Order: lane l of the replica's wave adds the
 *     selected entries l, l + 64, ... in that order, the 64 lane sums are added in a fixed order
 *     (as mmc_batch_dipoles), and boltz_sum's is added to the caller's value last: bitwise
 *     reproducible, whatever the grid or option "wave_wgs".
 *   - Sum rules (sel == NULL, no flags): every pair is counted from both of its molecules, and
 *     potential()'s totals count it once (energy.jl:978-980 and :1001 halve the sums over molecules), so
 *     esum[r][0] == 2 lj and esum[r][1] == 2 real of mmc_batch_potential_ewald's totals of the
 *     replica, up to summation order; esum[r][3] == N.
 *   - du_out [R][n][3] = (d_lj, d_real, d_recip).  Each output may be NULL, but not all of them.
 *   - Read-only: coordinates, S(k), the chains' flags, step counters and random streams are not
 *     touched; a chain run with these calls interleaved is bit-identical to one without.
 * MMC_ERR_STATE as mmc_batch_widom: proposals outstanding, a volume trial in flight, S(k) stale
 * after Wolf-style moves (call mmc_batch_recip_long), a run that failed half-way.
 * MMC_ERR_UNSUPPORTED, nothing computed: per-replica boxes (mmc_batch_set_boxes), Wolf style, a
 * system the table kernels do not take (not identical 3-atom molecules, or a cutoff / kappa
 * outside the erfc table), fewer than 2 molecules.  MMC_ERR_ARG: temperature <= 0 or not finite;
 * every output NULL; hist given with n_bins outside 1..4096, u_lo >= u_hi or a bound not finite;
 * sel given with n_sel < 1 or an index outside 0..N-1.  On any error every output is untouched. */
/* (`temperature` is this call's own argument: the batch's per-replica temperatures,
 * mmc_batch_set_temperatures, are not read) */
int32_t mmc_batch_deletion(mmc_batch *b, int32_t n_sel, const int32_t *sel, double temperature,
                           int32_t n_bins, double u_lo, double u_hi, int32_t per_replica,
                           uint64_t *hist      /* [n_bins + 2] or [R][n_bins + 2]; may be NULL */,
                           double *esum        /* [R][4] may be NULL */,
                           double *boltz_sum   /* [R] in/out, may be NULL */,
                           int64_t *n_flagged  /* [R] in/out, may be NULL */,
                           double *du_out      /* [R][n][3] may be NULL */,
                           uint8_t *ovl_out    /* [R][n] may be NULL */);

/* ---- Forces and torques on every molecule of every replica in one read-only pass ----------------
 * The reference has no forces beyond `fab` in LJ_poly_dU (Ewald/energy.jl:279-281).  Forces are
 * DEFINED as minus the gradient of its own total, potential(..., "ewald") (Ewald/energy.jl:946-1032),
 * at fixed neighbour sets: the COM gates r_ij^2 < r_cut^2 (energy.jl:254, ewalds.jl:340) and the atom
 * slack + 100 (energy.jl:270, ewalds.jl:362) decide which pairs count and are not differentiated --
 * exactly what a finite difference of the reference gives when atoms move and the stored COM array
 * does not.  For atom a of molecule i and atom b of a gated molecule j, rab = vector1D(ra, rb)
 * (boundaries.jl:8-14: b - a, minimum image) and r^2 = (x x + y y) + z z, unfused as everywhere:
 *   Lennard-Jones (energy.jl:270-281; eps > 0.001 and r^2 < r_cut^2 + 100), s2 = sigma^2 / r^2,
 *   s6 = s2^3, s12 = s6^2:
 *     f_a -= 24 eps (2 s12 - s6) / r^2 * rab
 *   Real-space Ewald (ewalds.jl:359-367; r^2 < r_cut^2 + 100):
 *     f_a -= factor q_a q_b (erfc(kappa r) / r + 2 kappa / sqrt(pi) exp(-kappa^2 r^2)) / r^2 * rab
 *     An atom pair of opposite charges with r^2 < 0.5 (:359-360) sets the overlap flag, as in
 *     mmc_batch_deletion.
 *   Reciprocal space (ewalds.jl:538-604; the batch's half-space list, doubled weights cfac_k, integer
 *   vectors n_k = (kx, ky, kz), k = 2 pi n / L):
 *     f_a += factor (4 pi / L) q_a sum_k cfac_k n_k Im(conj(S_k) e_{a,k})
 *     e_{a,k} = exp(i k . r_a) by the reference's phase recurrence, S_k the replica's committed
 *     structure factor (mmc_batch_recip_long, kept by the moves since).  Molecule i's own atoms are in
 *     S_k: this includes its interaction with itself that the reference's energy includes; EwaldSelf
 *     (:829-833) has no gradient.
 * Per molecule, with d_a = vector1D(COM_i, r_a) and the stored COM the point the library's rotations
 * turn about:
 *   F_i    = (f_0 + f_1) + f_2
 *   tau_i  = sum_a d_a x f_a, atoms in index order
 *   w_lj,i = the `vir` of LJ_poly_dU(i) in its own normalisation (energy.jl:281, :289):
 *            (24 / 3) sum_j sum_ab rij . (rab eps (2 s12 - s6) s2), rij = vector1D(COM_i, COM_j) --
 *            the reference's fab carries s2 = sigma^2 / r^2 where a force has 1 / r^2
 *   w_real,i = (1 / 3) sum_j rij . sum_ab factor q_a q_b (erfc(kappa r) / r + 2 kappa / sqrt(pi)
 *            exp(-kappa^2 r^2)) / r^2 * rab: the same form with the real-space Coulomb pair force
 *   t_i    = tau' I^-1 tau when mass [3] (per atom slot, > 0) is given, I = sum_a m_a (|d_a|^2 1 -
 *            d_a d_a'), the inverse by cofactors; else 0
 *   - Selection: as mmc_batch_deletion.  sel [n_sel] 0-based molecules, the same for every replica,
 *     duplicates allowed; sel == NULL: all N in index order (n_sel is ignored).  n = n_sel, or N.
 *   - Flags (ovl_out [R][n]): mmc_batch_widom's bits.  Bit 0 = overlap, bit 1 = some output of the
 *     molecule is not finite (an atom exactly on another, or a singular I: collinear sites).  A
 *     flagged molecule has zeros in every row, enters no sum and counts in n_flagged[r] (+=).
 *   - Rows: force_out [R][n][3] = F, torque_out [R][n][3] = tau, vir_out [R][n][3] = (w_lj, w_real,
 *     t), atom_out [R][n][3][3] = f_a.  Units: K / A, K, K (t: K^2 / (mass unit A^2)).
 *   - Order of summation within a molecule.  Pair part: lane l of the molecule's wave takes the
 *     gated-list entries l, l + 64, ... (molecules inside the 16-bit COM prefilter in ascending
 *     index, flushed when the list fills) and adds, per neighbour, the atom pairs a = 0..2, b = 0..2
 *     in that order to its sums; the 64 lane sums are added in a fixed order (as mmc_batch_dipoles).
 *     Reciprocal part: lane l adds k = l, l + 64, ...; same fixed order over the lanes.
 *     f_a = pair sum + (factor (4 pi / L) q_a) * reciprocal sum.
 *   - fsum [R][9], overwritten: (number summed, sum F.F, sum tau.tau, sum t, sum F_x, sum F_y,
 *     sum F_z, sum w_lj, sum w_real) over the replica's unflagged selected molecules, every product
 *     (x x + y y) + z z unfused.  Lane l of the replica's wave adds the entries l, l + 64, ... in
 *     that order and the 64 lane sums are added in a fixed order (mmc_batch_deletion's order):
 *     bitwise reproducible, whatever the grid or option "wave_wgs".
 *   - Sum rules (sel == NULL, no flags): sum_i F_i vanishes up to rounding (a pair's gate is the same
 *     from both sides, and the reciprocal forces sum to n_k Im(conj(S_k) S_k) = 0).  Every pair is
 *     counted from both of its molecules and potential()'s totals halve the sum over molecules
 *     (energy.jl:978-980), so fsum[r][7] == 2 (virial - coulomb / 3) of mmc_batch_potential_ewald's
 *     totals of the replica (its `virial` carries a third of every Coulomb term besides, :1001-1032),
 *     as esum[r][0] == 2 lj for mmc_batch_deletion.
 *   - Read-only: coordinates, S(k), the chains' flags, step counters and random streams are not
 *     touched; a chain run with these calls interleaved is bit-identical to one without.
 * MMC_ERR_STATE as mmc_batch_deletion: proposals outstanding, a volume trial in flight, S(k) stale
 * after Wolf-style moves (call mmc_batch_recip_long), a run that failed half-way.
 * MMC_ERR_UNSUPPORTED, nothing computed: per-replica boxes (mmc_batch_set_boxes), Wolf style, a
 * system the table kernels do not take (not identical 3-atom molecules, or a cutoff / kappa outside
 * the erfc table), fewer than 2 molecules.  MMC_ERR_ARG: every output NULL; sel given with
 * n_sel < 1 or an index outside 0..N-1; a mass <= 0 or not finite.  On any error every output is
 * untouched. */
int32_t mmc_batch_forces(mmc_batch *b, int32_t n_sel, const int32_t *sel, const double *mass /* [3] or NULL */,
                         double *force_out  /* [R][n][3]    may be NULL */,
                         double *torque_out /* [R][n][3]    may be NULL */,
                         double *vir_out    /* [R][n][3] = (w_lj, w_real, t)  may be NULL */,
                         double *atom_out   /* [R][n][3][3] f_a  may be NULL */,
                         double *fsum       /* [R][9]       may be NULL */,
                         int64_t *n_flagged /* [R] in/out   may be NULL */,
                         uint8_t *ovl_out   /* [R][n]       may be NULL */);

/* ---- Structure observables: site-site pair histograms and total dipole moments ----------------
 * mmc_batch_rdf_sites: what mmc_batch_rdf computes for one site, for all six unordered atom-slot
 * pairs of 3-site molecules in one pass, per replica if wanted, in either box mode.  Kept from
 * Ewald/gr.jl `makeRDF` (:68-92): the pair loop i < j with the difference site(i) - site(j), its
 * minimum image (:75-80: strict < -side/2 -> + side, > side/2 -> - side), r = sqrt((xx xx + yy yy)
 * + zz zz) unfused, bin = ceil(r / dr) (:87), counted when bin <= numbins (:88-90), and for
 * r_max <= 0 its bin width dr = side / 2 / numbins (:5).  Not kept: its one site per molecule, its
 * single frame, and its normalisation (observables.py: normalize_rdf_pairs).
 *   - Rows, in this order: slot pairs (0,0) (0,1) (0,2) (1,1) (1,2) (2,2).  Row (a,a) counts atom a
 *     of molecule i against atom a of molecule j for every i < j; row (a,b), a < b, counts both
 *     i.a - j.b and i.b - j.a.  Intermolecular pairs only.  Slots are positions in the molecule
 *     (SPC/E: O, H, H); folding rows by atom type is the host's (observables.py: fold_by_type).
 *   - r_max <= 0: dr = (L / 2) / numbins, one shared box only.  r_max > 0: dr = r_max / numbins;
 *     r_max must not exceed half of the smallest box of the batch.  With per-replica boxes
 *     (mmc_batch_set_boxes) each replica takes its own L for the image and all share dr; every box
 *     is >= 2 r_cut, so r_max = r_cut is always valid there.
 *   - per_replica == 0: hist[6][numbins + 1], summed over the replicas, like mmc_batch_rdf;
 *     per_replica != 0: hist[R][6][numbins + 1].  hist is overwritten, not accumulated.  Counter 0
 *     of a row only counts coincident sites.  The counts are exactly those of the arithmetic above
 *     (the kernel finds the bin from thresholds on r^2 built with it), whatever the grid or option
 *     "wave_wgs".
 * mmc_batch_dipoles: dip[R][3], M_r = sum_i mu_i in e A, mu_i = (q_0 d_0 + q_1 d_1) + q_2 d_2 per
 * component, unfused, d_a = the minimum image (vector1D, boundaries.jl, the replica's own box) of
 * atom a minus the molecule's centre of mass -- a molecule whose atoms are stored a box away from
 * its COM gives what the whole one gives.  Lane l of the replica's wave adds the molecules l,
 * l + 64, ... in that order and the 64 lane sums are added in a fixed order: bitwise reproducible,
 * independent of the launch.  Both box modes.
 * Both calls are read-only: coordinates, S(k), flags, step counters and random streams are not
 * touched; a chain with these calls between its blocks is bit-identical to one without.
 * Preconditions as mmc_batch_potential_ewald: no proposals outstanding (MMC_ERR_STATE), no volume
 * trial in flight (MMC_ERR_STATE).  MMC_ERR_ARG: numbins < 1 (or above 2046, what one wave's
 * histograms may take of a workgroup's LDS), a NULL output, r_max not finite, above half of the
 * smallest box, or <= 0 with per-replica boxes.  MMC_ERR_UNSUPPORTED: mmc_batch_rdf_sites with
 * more than 2^21 molecules.  (A batch holds three-atom molecules only, mmc_batch_create, so slots
 * 0..2 exist in every molecule.)  On any error the output is left untouched. */
int32_t mmc_batch_rdf_sites(mmc_batch *b, int32_t numbins, double r_max, int32_t per_replica,
                            uint64_t *hist);
int32_t mmc_batch_dipoles(mmc_batch *b, double *dip /* [R][3] */);

/* ---- Orientational pair correlations: h110(r), h112(r), <P2>(r) and the Kirkwood factor G_K(r) ---
 * The orientation-resolved pair pass between mmc_batch_rdf_sites (separations only) and
 * mmc_batch_local_order (orientation, first shell only): what the epsilon of the dipole fluctuation
 * (mmc_batch_dipoles) is made of, distance by distance.  The reference has no such analysis; the
 * arithmetic is defined here, in unfused fp64, and restated in numpy by tests/orient_ref.py.  Every
 * pair i < j of molecules of every replica contributes once.
 *   - Separation and bin: exactly row (0,0) of mmc_batch_rdf_sites.  d = site0(i) - site0(j) per
 *     component, its image gr.jl:75-80 with the replica's own box, r^2 = (xx xx + yy yy) + zz zz,
 *     bin = ceil(sqrt(r^2) / dr); dr and the validity of r_max as mmc_batch_rdf_sites in both box
 *     modes.  Bins 0..numbins are in range; slot numbins + 1 takes every pair beyond r_max and,
 *     unlike mmc_batch_rdf_sites, is returned.
 *   - Axis u_i of molecule i: mu_i as mmc_batch_dipoles computes it, (q_0 d_0 + q_1 d_1) + q_2 d_2
 *     with d_a = vector1D (boundaries.jl) of atom a minus the COM; n^2 = (mu_x^2 + mu_y^2) + mu_z^2,
 *     u = mu / sqrt(n^2), and u = 0 when n^2 is 0 or not finite.
 *   - Per pair: c = (u_i.x u_j.x + u_i.y u_j.y) + u_i.z u_j.z; p2 = 1.5 c^2 - 0.5;
 *     hd = 3 (u_i . d)(u_j . d) / r^2 - c, and hd = 0 when r^2 = 0 (dot products as c).
 *   - Rows: 0 the pair count; 1, 2, 3 the sums of Q(c), Q(hd), Q(p2) with Q(v) = v 2^30
 *     (MMC_ORIENT_SCALE) rounded to the nearest integer, ties to even, as a 64-bit integer.  In slot
 *     numbins + 1 rows 0 and 1 are filled, rows 2 and 3 are 0.  hd is evaluated with a per-pair error
 *     below 2^-31 (a refined reciprocal of r^2): a row-2 entry may differ from the exact arithmetic
 *     above by at most one unit per pair of its slot.
 *   - All four rows are integer sums: the result does not depend on the grid, on option "wave_wgs",
 *     on the flush order or on the order of atomics -- bitwise reproducible with no ordered
 *     reduction, at the price of a 2^-30 quantum per pair.  |Q| <= 2^31: the sums cannot wrap.
 *   - per_replica == 0: hist[4][numbins + 2] summed over the replicas; else hist[R][4][numbins + 2].
 *     hist is overwritten, not accumulated.
 *   - Use: G_K(R) = 1 + 2 sum_{bins <= R} row1 / (2^30 N frames), whose last element (slot
 *     numbins + 1 included) is the whole-box <|sum_i u_i|^2> / N; h110, h112 = rows 1, 2 over the
 *     ideal-gas pair count of the shell; <P2>(r) = row3 / (2^30 row0) (observables.py: kirkwood_gk,
 *     orient_projections).
 * Both box modes and either Coulomb style: the call reads coordinates and charges only, no S(k) and no
 * erfc table, and is read-only as mmc_batch_rdf_sites is.  Preconditions as mmc_batch_rdf_sites: no
 * proposals outstanding, no volume trial in flight (MMC_ERR_STATE).  MMC_ERR_ARG: numbins < 1 or above
 * MMC_ORIENT_MAX_BINS, a NULL hist, r_max not finite, above half of the smallest box, or <= 0 with
 * per-replica boxes.  MMC_ERR_UNSUPPORTED: more than 2^21 molecules.  Arguments are checked first,
 * then the state, then the size.  On any error hist is left untouched. */
int32_t mmc_batch_orient_corr(mmc_batch *b, int32_t numbins, double r_max, int32_t per_replica,
                              int64_t *hist /* [4][numbins + 2] or [R][4][numbins + 2] */);
#define MMC_ORIENT_SCALE 1073741824.0 /* 2^30: one unit of rows 1..3 */
/* What one wave per workgroup fits in the 65536 bytes of LDS a workgroup may ask for: the bin
 * thresholds, 8 (numbins + 2) bytes, and four 64-bit rows, 32 (numbins + 2) bytes:
 * 40 (numbins + 2) <= 65536  ->  numbins + 2 <= 1638. */
#define MMC_ORIENT_MAX_BINS 1636

/* ---- Spatial distribution functions: g(x, y, z) around a molecule in its own frame ----------------
 * The density of the neighbours' sites around a molecule in that molecule's body-fixed frame: the
 * donor caps in front of the hydrogens, the acceptor band behind the oxygen and the interstitial lobe
 * of water (Svishchev and Kusalik's maps).  mmc_batch_rdf_sites and mmc_batch_orient_corr integrate
 * these angles away; only a pass over all pairs with each molecule's frame in hand gives them.  The
 * reference has no such analysis; the arithmetic is defined here, in unfused fp64 (every operation
 * below is one fp64 operation in the order written, divisions and square roots IEEE), and restated in
 * numpy by tests/sdf_ref.py.  dot(a,b) = (a.x b.x + a.y b.y) + a.z b.z.
 *   - Frame of a molecule with sites s0, s1, s2 (slot 0 = O for water): o1 = vector1D(s0, s1) and
 *     o2 = vector1D(s0, s2) per component (boundaries.jl, the replica's own box; site a minus site 0),
 *     o0 = 0.  b = o1 + o2, h = o2 - o1.  nb2 = dot(b,b), e_z = b / sqrt(nb2).  t = dot(h, e_z),
 *     g = h - t e_z (multiply, then subtract).  ng2 = dot(g,g), e_x = g / sqrt(ng2).
 *     e_y = e_z x e_x, each component a difference of two products (e_y.x = e_z.y e_x.z - e_z.z e_x.y,
 *     and cyclic).  The molecule has no frame when nb2 or ng2 is 0 or not finite (a NaN included).
 *   - Per pair i < j of a replica: d = vector1D(s0(i), s0(j)) per component; as seen from j the
 *     vector is -d bit for bit, it is not recomputed.  For every slot a selected in site_mask (bit a)
 *     two deposits are made.  Into i's frame: w = d + o_a(j),
 *     p = (dot(e_x(i), w), dot(e_y(i), w), dot(e_z(i), w)).  Into j's frame: w' = -d + o_a(i),
 *     projected on j's axes.
 *   - Folding and cells.  fold bit 0 replaces p.x by |p.x|, bit 1 replaces p.y by |p.y| (both are
 *     symmetries of C2v water); z is never folded.  The cell edges are e_k = (double)k * cell,
 *     k = -n_half .. n_half.  Along an unfolded axis p lies in cell k when e_k <= p < e_k+1, stored
 *     at index k + n_half: 2 n_half cells.  Along a folded axis there are n_half cells,
 *     k = 0 .. n_half - 1.  A deposit is outside when any coordinate falls in no cell; a NaN counts
 *     as outside.  Flat index (ix g_y + iy) g_z + iz, with g_z = 2 n_half.
 *   - Counters: one 64-bit count per cell, then `outside`, then `noframe`: a centre molecule without
 *     a frame sends all of its deposits there.  So per replica
 *     cells + outside + noframe = N (N - 1) popcount(site_mask) exactly.
 *   - All counts are integers: the result does not depend on the grid, on option "wave_wgs", on the
 *     flush order or on the order of atomics.
 *   - per_replica == 0: hist[g_x g_y g_z + 2] summed over the replicas; else hist[R][g_x g_y g_z + 2].
 *     hist is overwritten, not accumulated.
 *   - Use: g = count / (frames N (N - 1) / V popcount(site_mask) cell^3 2^(folded axes))
 *     (observables.py: sdf_density, sdf_unfold, sdf_cell_centres).
 * Both box modes, either Coulomb style, records or arrays: the call reads coordinates only and is
 * read-only as mmc_batch_orient_corr is, with its preconditions: no proposals outstanding, no volume
 * trial in flight (MMC_ERR_STATE).  MMC_ERR_ARG: a NULL hist, n_half < 1, cell not finite or <= 0,
 * fold outside 0..3, site_mask outside 1..7, g_x g_y g_z > MMC_SDF_MAX_CELLS, or a cube that reaches
 * another periodic image: required is sqrt(3) n_half cell + rho <= L_min / 2 with L_min the smallest
 * box and rho = 2 r_mol_max, r_mol_max being the batch's bound on the distance of any site from its
 * molecule's centre of mass (DeviceSystem::r_mol_max: the uploaded and every set configuration, the
 * body-fixed sites of mmc_batch_set_orientations; unknown, and the call refused, once the caller has
 * proposed moves of its own).  |o_a| <= rho, so under this condition every site inside the cube
 * belongs to the minimum image of the O-O vector.  MMC_ERR_UNSUPPORTED: more than 2^21 molecules, or a
 * device that grants a workgroup less LDS than the grid needs.  The arguments that need no batch are
 * checked first, then the state, then the cube against the boxes, then the size.  On any error hist
 * is left untouched. */
int32_t mmc_batch_sdf(mmc_batch *b, int32_t n_half, double cell, int32_t fold, int32_t site_mask,
                      int32_t per_replica, uint64_t *hist /* [g_x g_y g_z + 2] or [R][...] */);
/* 32-bit counters in the LDS of one workgroup: 4 x 32768 = 128 KB of the 160 KB a gfx950 workgroup
 * may claim, the cell edges and the scaffold beside them. */
#define MMC_SDF_MAX_CELLS 32768

/* ---- Pair-energy distributions: p(u), <u_C>(r), <u_LJ>(r) and energetic hydrogen bonds -----------
 * The energy of a PAIR of molecules, which no other call exports (mmc_batch_deletion sums over the
 * partners, mmc_batch_rdf_sites has no energies, mmc_batch_local_order counts bonds by geometry): the
 * distribution p(u) of dimer interaction energies, the decomposition of the potential energy by
 * distance, and the hydrogen-bond count of the energetic criterion u < u_hb (Jorgensen: -2.25
 * kcal/mol = -1132.2 K).  The reference has no such analysis; the arithmetic is defined here, in
 * unfused fp64, and restated in numpy by tests/pair_energy_ref.py.  Every pair i < j of three-site
 * molecules of every replica contributes once.  Energies are in K.
 *   - Separation and r-bin: exactly mmc_batch_orient_corr's.  D = site0(i) - site0(j) per component,
 *     its image gr.jl:75-80 with the replica's own box, r^2 = (xx xx + yy yy) + zz zz,
 *     bin = ceil(sqrt(r^2) / dr) from the host-built thresholds; dr and the validity of r_max as
 *     mmc_batch_rdf_sites in both box modes.  Bins 0..numbins are in range; slot numbins + 1 takes
 *     every pair beyond r_max.
 *   - Molecule image.  e_a(m) = vector1D(site 0 of m, atom a of m) (boundaries.jl) per component with
 *     the replica's own box, so e_0 = 0 and a molecule whose atoms are stored a box apart is whole.
 *     The atom-pair vector is x_ab = (D + e_a(i)) - e_b(j) per component, r2_ab = (x x + y y) + z z.
 *     The cutoff is by molecule: all nine atom pairs of a pair in range count, with no atomic cutoff.
 *   - Energies of a pair in range, a = 0, 1, 2 major and b = 0, 1, 2 minor, each sum added left to
 *     right in that order:
 *         u_C  = factor * (sum_ab (q_a * q_b) / sqrt(r2_ab))
 *         u_LJ = sum_ab (4.0 * eps_ab) * (s6 * s6 - s6),  s6 = (s2 * s2) * s2,
 *                s2 = (sig_ab * sig_ab) / r2_ab, over the atom pairs with eps_ab > 0.001 (the
 *                reference's LJ rule, energy.jl:270; quirk Q2), 0 when there is none
 *         u    = u_C + u_LJ
 *     with q_a the charge of atom a of i, q_b of atom b of j, eps and sig the tables at (type of a,
 *     type of b), factor the Coulomb constant of the batch.  The device may evaluate u_C and u_LJ of
 *     an unflagged pair to within 2^-21 K of this arithmetic (refined reciprocal square roots for the
 *     divisions).
 *   - Flagged pairs.  A pair in range whose u_C or u_LJ is not finite or has magnitude >= 2^20 K
 *     (atoms on top of each other) is counted in flagged and in row 0 and enters no other output.
 *   - rows: 0 the pair count per slot; 1 and 2 the sums of Q(u_C) and Q(u_LJ) over the unflagged
 *     pairs of bins 0..numbins, Q(v) = v 2^20 (MMC_PAIRE_SCALE) rounded to the nearest integer,
 *     ties to even, as a 64-bit integer; rows 1 and 2 of slot numbins + 1 are 0: pairs beyond r_max
 *     compute no energy.  A row-1 or row-2 entry may differ from the exact arithmetic above by at
 *     most one unit per pair of its slot.  The sums are integers, added modulo 2^64: a slot is right
 *     whenever its true sum is below 2^43 K in magnitude (ask per replica where a summed call could
 *     pass that), and the result does not depend on the grid, on option "wave_wgs", on the flush
 *     order or on the order of atomics.
 *   - uhist: every unflagged pair in range, binned on u by mmc_batch_deletion's rule: with
 *     s = n_ebins / (u_hi - u_lo) in fp64 and k = floor((u - u_lo) * s), unfused, u < u_lo goes to
 *     slot 0, u >= u_hi or k >= n_ebins to slot n_ebins + 1, everything else to slot k + 1
 *     (observables.energy_bins).
 *   - nhb: c_m = the number of unflagged partners of molecule m in range with u < u_hb; nhb[k] = the
 *     number of molecules with c_m = k, the last slot MMC_PAIRE_NHB - 1 = 8 taking c_m >= 8.
 *   - per_replica == 0: rows[3][numbins + 2], uhist[n_ebins + 2], nhb[MMC_PAIRE_NHB], flagged[1],
 *     summed over the replicas; else rows[R][3][numbins + 2], uhist[R][n_ebins + 2],
 *     nhb[R][MMC_PAIRE_NHB], flagged[R].  All are overwritten, not accumulated.  uhist and nhb may be
 *     NULL; without uhist n_ebins, u_lo and u_hi are ignored, without nhb u_hb is.
 *   - Use (observables.py): pair_energy_distribution, pair_energy_profile, energetic_hbonds.
 * Both box modes and either Coulomb style: the call reads coordinates, charges and the eps / sig
 * tables only, no S(k) and no erfc table (the pair energy is the bare Coulomb one in both styles), and
 * is read-only as mmc_batch_rdf_sites is.  Arguments are checked first, then the state, then the
 * size; on any error every output is left untouched.  MMC_ERR_ARG, before the batch is looked at:
 * NULL rows or NULL flagged; numbins outside 1..MMC_PAIRE_MAX_BINS; r_max not finite; uhist given
 * with n_ebins outside 1..MMC_PAIRE_MAX_EBINS, u_lo >= u_hi or a bound that is not finite; nhb given
 * with u_hb not finite; with the batch: r_max above half of the smallest box, or <= 0 with
 * per-replica boxes.  MMC_ERR_STATE: proposals outstanding, a volume trial in flight.
 * MMC_ERR_UNSUPPORTED: molecules that are not three-site; more than 2^21 molecules. */
int32_t mmc_batch_pair_energy(mmc_batch *b, int32_t numbins, double r_max,
        int32_t n_ebins, double u_lo, double u_hi, double u_hb, int32_t per_replica,
        int64_t *rows     /* [3][numbins + 2] or [R][3][numbins + 2] */,
        uint64_t *uhist   /* [n_ebins + 2]    or [R][n_ebins + 2];   may be NULL */,
        uint64_t *nhb     /* [MMC_PAIRE_NHB]  or [R][MMC_PAIRE_NHB]; may be NULL */,
        uint64_t *flagged /* [1] or [R] */);
#define MMC_PAIRE_SCALE 1048576.0 /* 2^20: one unit of rows 1 and 2 */
#define MMC_PAIRE_NHB 9           /* molecules with 0..7 energetic bonds, then 8 or more */
#define MMC_PAIRE_MAX_EBINS 4096  /* largest n_ebins (mmc_batch_deletion's) */
/* What one wave per workgroup fits in the 65536 bytes of LDS a workgroup may ask for, all counters
 * 64-bit: the bin thresholds, 8 (numbins + 2) bytes, three rows, 24 (numbins + 2) bytes, the LJ
 * constants of the nine atom pairs, 144 bytes, the largest energy histogram,
 * 8 (MMC_PAIRE_MAX_EBINS + 2) bytes, and the flagged count, 8 bytes:
 * 32 (numbins + 2) + 144 + 32784 + 8 <= 65536  ->  numbins + 2 <= 1018. */
#define MMC_PAIRE_MAX_BINS 1016

/* ---- Partial structure factors: S_ab(q) and the charge structure factor S_ZZ(q) of every replica ---
 * The reciprocal-space counterpart of mmc_batch_rdf_sites: the products rho_a(n) rho_b(n)* of the three
 * atom-slot densities over the box's own wave vectors, summed per shell of |n|^2, in one read-only
 * pass.  What mmc_batch_recip_long builds for the 337 Ewald vectors, charge-weighted and only as an
 * energy (Ewald/ewalds.jl:538-604, the powers :575-585), is built here per slot out to |n| <= 32.
 * The arithmetic is defined here, in unfused fp64, and restated in numpy by tests/sofq_ref.py.
 *   - Vectors and shells.  n = (nx, ny, nz) integer with 0 < s = nx^2 + ny^2 + nz^2 <= n_max^2;
 *     q = 2 pi n / L with L the replica's own box; the shell index is s.  count[s] is the number of
 *     all such vectors, r_3(s): 0 for empty shells and for s = 0.  The kernel visits the half space
 *     (nx > 0, or nx = 0 and ny > 0, or nx = ny = 0 and nz > 0) and doubles each contribution:
 *     rho(-n) = conj rho(n), so doubling is exact.
 *   - Slot densities.  rho_a(n) = sum_i e^{i 2 pi n . r_{i,a} / L} over the molecules i, for atom
 *     slot a = 0, 1, 2 (a batch holds three-atom molecules only).  The stored coordinates are used
 *     with no imaging: the phase is periodic.
 *   - Phase arithmetic: k_recip_long_lds' (csrc/mmc_total.hpp).  Per component (cos, sin) of
 *     2 pi x / L by sincos_moderate (csrc/mmc_device.hpp); powers by repeated c_mul, p_0 = 1,
 *     p_k = c_mul(p_{k-1}, e1) (the first product, 1 e1, is exact); negative indices by conjugation;
 *     product order (x y) z: the term of atom (i, a) is c_mul(c_mul(ex, ey), ez).
 *   - Summation order.  Lane l of one wave adds the molecules l, l + 64, ... in that order, the 64
 *     lane sums go through wave_sum (csrc/mmc_device.hpp: lane l += lane l + 32, 16, 8, 4, 2, 1), and
 *     one wave computes a given rho_a(n) alone: the bits of every rho do not depend on the launch.
 *   - Rows, in mmc_batch_rdf_sites' order: slot pairs (0,0) (0,1) (0,2) (1,1) (1,2) (2,2).  Per
 *     half-space vector v_ab = rho_a.re rho_b.re + rho_a.im rho_b.im, unfused; Q(v) = v 2^24
 *     (MMC_SOFQ_SCALE) rounded to the nearest integer, ties to even, as a 64-bit integer;
 *     sq[r][row][s] = 2 sum over the half-space vectors n of shell s of Q(v_ab(n)).  Row (a,b), a < b,
 *     holds the cross term once: the host doubles it when it forms |sum_a w_a rho_a|^2.  Self terms
 *     and intramolecular terms are included: S_aa -> 1 at large q.
 *   - All sums are integers: no order of waves, atomics or flushes can change a bit, whatever the
 *     grid or option "wave_wgs".  N <= 2^10 and count <= 552 give |sq| < 2^54: the sums cannot wrap.
 *   - per_replica != 0: sq[R][6][n_max^2 + 1], overwritten; sq_sum must be NULL.  per_replica == 0:
 *     sq_sum[row][s] = sum over r = 0 .. R - 1, ascending, of (double)sq[r][row][s] 2^-24 in fp64,
 *     added in that order; sq must be NULL.  Bitwise reproducible.  count [n_max^2 + 1] may be NULL.
 *   - Use (observables.py): S_ab(q) = <rho_a rho_b*> / sqrt(N_a N_b) averaged over the shell's
 *     vectors (partial_structure_factors), S_ZZ = <|sum_a q_a rho_a|^2> / N (charge_structure_factor),
 *     1 - 1 / eps_L(q) = 4 pi beta N S_ZZ / (V q^2) (dielectric_longitudinal).
 * Both box modes and either Coulomb style: the call reads coordinates only, and is read-only as
 * mmc_batch_rdf_sites is.  Preconditions as mmc_batch_rdf_sites: no proposals outstanding, no volume
 * trial in flight (MMC_ERR_STATE).  MMC_ERR_ARG, checked before the batch: n_max outside
 * 1..MMC_SOFQ_MAX_N, the output that per_replica selects NULL, the other output given; checked with
 * the batch: per_replica == 0 with per-replica boxes (equal s are different q there: ask per
 * replica).  MMC_ERR_UNSUPPORTED: more than MMC_SOFQ_MAX_MOL molecules.  Arguments are checked first,
 * then the state, then the size.  On any error every output is left untouched. */
#define MMC_SOFQ_MAX_N   32            /* largest n_max */
#define MMC_SOFQ_MAX_MOL 1024          /* largest N: the phases of 3 N atoms stay in one workgroup's LDS */
#define MMC_SOFQ_SCALE   16777216.0    /* 2^24: one unit of sq */
int32_t mmc_batch_structure_factor(mmc_batch *b, int32_t n_max, int32_t per_replica,
                                   int32_t *count /* [n_max*n_max + 1] may be NULL */,
                                   int64_t *sq    /* [R][6][n_max*n_max + 1], per_replica != 0; may be NULL */,
                                   double  *sq_sum/* [6][n_max*n_max + 1],    per_replica == 0; may be NULL */);

/* ---- Local order: hydrogen bonds and the tetrahedral order parameter of 3-site molecules ------
 * The first coordination shell of every molecule of every replica in one read-only pass.  Slot 0 of
 * a molecule is the heavy atom ("O"), slots 1 and 2 are the hydrogens: the order of every water deck
 * here.  The reference has no such analysis; the arithmetic is defined here and restated in numpy by
 * tests/local_order_ref.py.
 *   d(x, y) is vector1D (Ewald/boundaries.jl; csrc/mmc_device.hpp): y - x, moved by one box when
 *   |d| >= L / 2, per component, with the replica's own box.  Every r^2 and every dot product is
 *   (x x' + y y') + z z' in unfused fp64.
 *   - Neighbours.  For molecule i every other molecule j has r2_ij = r^2 of d(O_i, O_j).  The four
 *     nearest are the four smallest under the key (bit pattern of r2_ij, then j): ties go to the
 *     lower index; rank 0 is the nearest.
 *   - Tetrahedral order (Errington and Debenedetti).  With d_a = d(O_i, O_a) for ranks a, b:
 *     c_ab = (d_a . d_b) / sqrt(r2_a r2_b); s = the sum of (c_ab + 1/3)^2 over (0,1) (0,2) (0,3)
 *     (1,2) (1,3) (2,3), added in that order; q_i = 1 - 0.375 s.  A molecule with a coincident
 *     neighbour (r2 == 0) has q_i = NaN, is counted in no bin and not in q_sum.  Its bin is
 *     k = min(q_bins - 1, max(0, (int)floor((q_i + 3.0) (q_bins / 4.0)))) over [-3, 1].
 *   - Hydrogen bonds (Luzar-Chandler geometry).  Donor i through its hydrogen h in {1, 2} to
 *     acceptor j != i: r2_ij < r_hb r_hb, and with u = d(O_i, H_i,h), v = d(O_i, O_j), t = u . v:
 *     t > 0 and t t >= cos_hb cos_hb (|u|^2 |v|^2).  No sqrt, division or trigonometry; pass
 *     cos_hb = cos(30 deg).  donated_i counts the pairs (h, j) with i the donor, accepted_i the pairs
 *     (j, h) with i the acceptor, total_i their sum; each of the three is clamped to 8.
 *   - Outputs, all overwritten, each may be NULL but not all of hb_hist, q_hist and q_sum:
 *     hb_hist [3][9] (rows donated, accepted, total; molecules over n = 0..8), [R][3][9] with
 *     per_replica; q_hist [q_bins], [R][q_bins] with per_replica; q_sum [R][2] = (the sum of the
 *     replica's finite q_i, their number as a double): lane l of the replica's wave adds the
 *     molecules l, l + 64, ... in that order and the 64 lane sums are added in a fixed order --
 *     bitwise reproducible, independent of the launch, like mmc_batch_dipoles; nbr_out [R][N][4]
 *     0-based j by rank; q_out [R][N]; hb_out [R][N][2] donated, accepted.  The counts do not depend
 *     on the grid or option "wave_wgs".
 * Both box modes and either Coulomb style: the call reads coordinates only, and is read-only as
 * mmc_batch_rdf_sites is (coordinates, S(k), flags, step counters and random streams are not
 * touched; S(k) need not be fresh).  Preconditions as mmc_batch_rdf_sites: no proposals
 * outstanding, no volume trial in flight, no run that failed half-way (MMC_ERR_STATE).
 * MMC_ERR_ARG: r_hb not finite, <= 0 or above half of the smallest box; cos_hb outside (0, 1];
 * q_bins outside 1..4096; hb_hist, q_hist and q_sum all NULL.  MMC_ERR_UNSUPPORTED: fewer than 5
 * molecules (no four neighbours) or more than 2^21.  On any error every output is left untouched. */
int32_t mmc_batch_local_order(mmc_batch *b, double r_hb, double cos_hb, int32_t q_bins,
                              int32_t per_replica, uint64_t *hb_hist, uint64_t *q_hist,
                              double *q_sum, int32_t *nbr_out, double *q_out, uint8_t *hb_out);

/* ---- Hydrogen-bond network: clusters, their sizes and percolation ------------------------------
 * How the hydrogen bonds of mmc_batch_local_order connect: the bond graph of every replica, its
 * connected components, the cluster-size distribution n_s and whether a cluster spans the periodic
 * box (Geiger, Stillinger and Rahman, J. Chem. Phys. 70, 4185, 1979; Stanley and Teixeira, J. Chem.
 * Phys. 73, 3404, 1980).  Up to MMC_NET_MAX_CRIT bond criteria per call, criterion k being
 * (r_hb[k], cos_hb[k], min_bonds[k]).  The reference has no such analysis; the definitions are
 * stated here and restated in numpy by tests/network_ref.py.  Every result is an integer: nothing is
 * left to a tolerance.
 *   - Bond.  A_k(i, j), i != j, holds when molecule i donates to j or j donates to i through either
 *     hydrogen; "donates" is exactly the test of "Local order" with (r_hb[k], cos_hb[k]): the same
 *     unfused fp64 arithmetic, vector1D images and replica box.  A_k is symmetric; two hydrogens to
 *     one partner, or donation both ways, are one bond.
 *   - Degree.  deg_k(i) = the number of j with A_k(i, j), over all molecules, before any selection.
 *   - Flagged.  A (replica, criterion) in which some molecule has deg_k > MMC_NET_MAX_DEG is flagged:
 *     it enters no histogram, its stats are 0 except stats[7] = 1, its labels are -2 and its partner
 *     lists -1 throughout (as mmc_batch_pair_energy's `flagged`).  It is not an error; other replicas
 *     and criteria are unaffected.
 *   - Sites and edges.  V_k = { i : deg_k(i) >= min_bonds[k] }: every molecule with min_bonds 0, the
 *     four-bonded ones with 4.  E_k = A_k restricted to V_k x V_k.
 *   - Clusters.  The connected components of (V_k, E_k); a site without edges is a cluster of size 1.
 *     The label of a site is the smallest molecule index of its cluster; other molecules have -1.
 *   - Wrapping.  For an edge (i, j), m_ij is the integer vector of boxes that vector1D adds per
 *     component to O_j - O_i (each -1, 0 or +1; m_ji = -m_ij bit for bit, because O_i - O_j is the
 *     exact negative of O_j - O_i).  A cluster wraps along axis a when it contains a closed walk over
 *     its edges whose sum of m has a nonzero component a; its mask has bit a set (x = 1, y = 2, z = 4).
 *     With p the sum of m along a spanning tree from the root, the mask is the OR over the edges of
 *     the nonzero components of p_i + m_ij - p_j.  It does not depend on the tree, on the order of
 *     traversal or on whether atoms are stored inside the box: the winding vectors of any spanning
 *     tree's non-tree edges generate the same sublattice (the windings of all closed walks), and
 *     storing a molecule one box over changes m on all its edges by the same vector, which cancels
 *     around every closed walk.
 *   - Outputs, all integers, all overwritten; each may be NULL, but not all three of size_hist,
 *     deg_hist and stats:
 *     size_hist uint64 [K][N + 1], [R][K][N + 1] with per_replica: entry s = the number of clusters
 *       of s sites; entry 0 stays 0.
 *     deg_hist uint64 [K][MMC_NET_MAX_DEG + 1], [R][K][..] with per_replica: molecules by deg_k, the
 *       f_j of the percolation papers.
 *     stats int64 [R][K][MMC_NET_STATS]: 0 bonds |A_k|; 1 sites |V_k|; 2 clusters; 3 the size of the
 *       largest cluster; 4 the sum of s^2 over the clusters; 5 the OR of the clusters' masks; 6 the
 *       size of the largest cluster with a nonzero mask (0 if none); 7 flagged (0 or 1).
 *     label_out int32 [R][K][N].
 *     nbr_out int32 [R][K][N][MMC_NET_MAX_DEG]: the partners under A_k in ascending j, then -1.
 *     Nothing depends on the grid, on option "wave_wgs" or on any order of lanes, waves or atomics.
 *   - Use (observables.py): cluster_size_distribution, percolation_probability, gel_fraction,
 *     mean_cluster_size, bond_fractions.
 * Both box modes and either Coulomb style, records or arrays: the call reads coordinates only, and is
 * read-only exactly as mmc_batch_local_order is, with its preconditions (MMC_ERR_STATE).
 * MMC_ERR_ARG, checked before the batch: n_crit outside 1..MMC_NET_MAX_CRIT; r_hb, cos_hb or
 * min_bonds NULL; an r_hb not finite or <= 0; a cos_hb outside (0, 1]; a min_bonds outside
 * 0..MMC_NET_MAX_DEG; size_hist, deg_hist and stats all NULL.  Checked with the batch: an r_hb above
 * half of the smallest box.  Then the state; then MMC_ERR_UNSUPPORTED: fewer than 2 molecules, or more
 * than MMC_NET_MAX_MOL (a replica's graph stays in one workgroup's LDS: 28 bytes per molecule and
 * 33 per molecule and criterion of a pass).  On any error every output is left untouched. */
#define MMC_NET_MAX_CRIT 8
#define MMC_NET_MAX_DEG  16
#define MMC_NET_STATS    8
#define MMC_NET_MAX_MOL  2048
int32_t mmc_batch_hbond_network(mmc_batch *b, int32_t n_crit, const double *r_hb, const double *cos_hb,
                                const int32_t *min_bonds, int32_t per_replica, uint64_t *size_hist,
                                uint64_t *deg_hist, int64_t *stats, int32_t *label_out, int32_t *nbr_out);

/* ---- Hydrogen-bond rings: shortest-path ring statistics -------------------------------------------
 * The topology of the hydrogen-bond network beyond its connectivity: the closed rings of bonds of
 * every replica, by size.  Ice Ih and Ic are all six-rings; the liquid shows a mix of 5, 6 and 7 that
 * shifts on supercooling.  Counted are the shortest-path rings of Franzblau (Phys. Rev. B 44, 4925,
 * 1991), as used for water by Matsumoto, Baba and Ohmine (J. Chem. Phys. 127, 134504, 2007).  One bond
 * criterion (r_hb, cos_hb) per call.  The reference has no such analysis; the definitions are stated
 * here and restated in numpy by tests/rings_ref.py.  Every result is an integer: nothing is left to a
 * tolerance.
 *   - Graph.  Exactly mmc_batch_hbond_network's for the criterion (r_hb, cos_hb): A(i, j) is its
 *     undirected bond (the same unfused fp64 arithmetic, vector1D images and replica box), D(i, j)
 *     means "i donates to j through either hydrogen" (A(i, j) = D(i, j) or D(j, i)), and m_ij is the
 *     bond's integer box vector (m_ji = -m_ij).  deg(i) = the number of j with A(i, j).
 *   - Flagged.  A replica in which some molecule has deg > MMC_RING_MAX_DEG is flagged: it enters no
 *     histogram, its stats are 0 except stats[7] = 1, its count_out entries are 65535 (-1 as uint16)
 *     and its ring_out rows -1.  It is not an error; other replicas are unaffected.  (The cap is below
 *     the network's 16 because the search grows with deg^(n/2); liquid water at the usual criteria has
 *     at most 5 or 6 bonds per molecule.)
 *   - Ring.  A cyclic sequence p_0 .. p_(n-1) of n distinct molecules, 3 <= n <= n_max <=
 *     MMC_RING_MAX_SIZE, with A(p_k, p_(k+1)) for every k cyclically.  It is a shortest-path ring when
 *     it has no shortcut: for every two members p_a, p_b the distance in the replica's finite graph
 *     of N molecules (the fewest bonds of any path, through members or not) equals their distance
 *     round the ring, min(|a - b|, n - |a - b|).  Each ring counts once, whatever its start and
 *     direction.  Only shortest-path rings are counted, here called rings.
 *   - Wrapping.  A ring wraps when the sum of m_(p_k p_(k+1)) round it is not (0, 0, 0): it closes
 *     through the periodic box and is an artefact of the box size.  Such rings are counted apart (row
 *     1, stats[2]) and enter nothing else.  The sum does not depend on whether atoms are stored
 *     inside the box (see "Hydrogen-bond network").
 *   - Homodromic.  A ring that does not wrap is homodromic when D(p_k, p_(k+1)) holds for every k
 *     cyclically, or D(p_(k+1), p_k) holds for every k: the donations run round it one way.
 *   - Canonical form.  The lowest member first, then the smaller of its two ring neighbours, then
 *     onward round the ring.
 *   - Outputs, all integers, all overwritten; each may be NULL, but not all three of ring_hist,
 *     member_hist and stats:
 *     ring_hist uint64 [3][MMC_RING_MAX_SIZE + 1], [R][3][..] with per_replica: row 0 the rings that
 *       do not wrap, by size; row 1 the wrapping rings by size; row 2 the homodromic ones among row 0.
 *       Entries 0, 1, 2 and those above n_max are 0.
 *     member_hist uint64 [MMC_RING_MAX_SIZE + 1][MMC_RING_MEMBER_BINS], [R][..] with per_replica: row
 *       n, bin c = the number of molecules that are members of c row-0 rings of size n; row 0 counts
 *       rings of any size; the last bin means "32 or more".  Rows 1, 2 and those above n_max are 0.
 *     stats int64 [R][MMC_RING_STATS]: 0 bonds |A|; 1 rings (row 0 summed); 2 wrapping rings; 3
 *       homodromic rings; 4 molecules in no row-0 ring; 5 the largest number of row-0 rings one
 *       molecule is a member of; 6 the row-0 rings that did not fit into ring_out (0 without
 *       ring_out); 7 flagged (0 or 1).
 *     count_out uint16 [R][N][MMC_RING_MAX_SIZE + 1]: per molecule the number of row-0 rings of each
 *       size it is a member of; entry 0 their total, entries 1 and 2 zero; saturating at 65535.
 *     ring_out int32 [R][max_rings][MMC_RING_MAX_SIZE]: the row-0 rings of replica r in canonical
 *       form, padded with -1; unused rows are -1 throughout.  Rings beyond max_rings are dropped and
 *       counted in stats[6]; which ones are dropped, and the order of the rows, is the one thing in
 *       the call that may depend on the launch.  max_rings is ignored when ring_out is NULL.
 *     Everything else is independent of the grid, of options "wave_wgs" and "ring_chunk" and of any
 *     order of lanes, waves or atomics.
 *   - Staging.  With count_out or ring_out the replicas are worked off in launches whose details
 *     stay under a fixed budget of device memory (256 MiB), one after the other on the batch's
 *     stream.  Option "ring_chunk" = n > 0 sets the replicas per launch (for tests of a ragged last
 *     one); 0 = by the budget.
 *   - Use (observables.py): ring_size_distribution, ring_fractions, homodromic_fraction,
 *     ring_membership.
 * Both box modes and either Coulomb style, records or arrays: the call reads coordinates only, and is
 * read-only exactly as mmc_batch_local_order is, with its preconditions (MMC_ERR_STATE).
 * MMC_ERR_ARG, checked before the batch: r_hb not finite or <= 0; cos_hb outside (0, 1]; n_max outside
 * 3..MMC_RING_MAX_SIZE; ring_hist, member_hist and stats all NULL; ring_out with max_rings < 1.
 * Checked with the batch: r_hb above half of the smallest box.  Then the state; then
 * MMC_ERR_UNSUPPORTED: fewer than 2 molecules, more than MMC_NET_MAX_MOL, or a device that does not
 * grant the LDS a replica's graph needs (57 bytes per molecule, and one more per molecule for each
 * of the workgroup's at least four waves).  On any error every output is left untouched. */
#define MMC_RING_MAX_SIZE    8
#define MMC_RING_MAX_DEG     8
#define MMC_RING_STATS       8
#define MMC_RING_MEMBER_BINS 33
int32_t mmc_batch_hbond_rings(mmc_batch *b, double r_hb, double cos_hb, int32_t n_max, int32_t per_replica,
                              uint64_t *ring_hist, uint64_t *member_hist, int64_t *stats,
                              uint16_t *count_out, int64_t max_rings, int32_t *ring_out);

/* ---- Shell order: ranked neighbours, LSI, zeta and O-O-O angles of 3-site molecules -----------
 * What lies between the first and the second coordination shell of every molecule of every replica,
 * in one read-only pass: the neighbour-rank decomposition of g_OO (row 5 is the distribution of the
 * fifth-neighbour distance d5), the local structure index (Shiratani and Sasai, J. Chem. Phys. 104,
 * 7671, 1996), zeta (Russo and Tanaka, Nat. Commun. 5, 3556, 2014) and the O-O-O angle distribution.
 * Slot 0 of a molecule is the heavy atom ("O"), slots 1 and 2 the hydrogens.  The reference has no
 * such analysis; the arithmetic is defined here, operation by operation, and restated in numpy by
 * tests/shell_order_ref.py.  + - x / sqrt floor are correctly rounded fp64 and nothing is fused, so
 * every output is reproducible bit for bit.
 *   d(x, y) is vector1D as in "Local order", per component, with the replica's own box.  Every r^2
 *   and every dot product is (x x' + y y') + z z'.  Squares of the radii (r_list r_list, ...) and
 *   the scales named below are formed once, in fp64, by the host.
 *   - List.  For molecule i: d_ij = d(O_i, O_j), r2_ij its r^2.  The list holds every j != i with
 *     r2_ij < r_list r_list, ascending under the key (bit pattern of r2_ij, then j).  m_i is its
 *     length, rho_k = sqrt(r2_k) the k-th distance, k = 1 .. m_i.  A list has room for
 *     MMC_SHELL_CAP = 64 neighbours.  A molecule with more in range is FLAGGED: counted in flagged[r],
 *     in no histogram and no sum; its count_out is -1, its nbr_out -1, its lsi_out and zeta_out NaN.
 *     A list is never truncated.  (64 neighbours reach to 7.7 A in water at 1 g/cm^3: the second
 *     shell ends at 5.7 A.)
 *   - Rank histograms.  For k = 1 .. n_rank the molecule adds one to row k - 1 of rank_hist
 *     [n_rank][r_bins + 1]: at bin min(r_bins - 1, (int)floor(rho_k inv_dr)), inv_dr = r_bins / r_list,
 *     or at slot r_bins when m_i < k.
 *   - LSI.  n = the number of listed neighbours with r2 < r_lsi r_lsi.  Defined when n >= 1 and
 *     m_i >= n + 1 (the neighbour just beyond r_lsi is in the list).  Delta_k = rho_(k+1) - rho_k,
 *     k = 1 .. n; mean = (Delta_1 + Delta_2 + ...) / n and I = ((Delta_1 - mean)^2 + (Delta_2 -
 *     mean)^2 + ...) / n, each sum added one term at a time in rising k, each square one product.
 *     Bin min(lsi_bins - 1, (int)floor(I lsi_scale)), lsi_scale = lsi_bins / lsi_max; undefined:
 *     slot lsi_bins of lsi_hist [lsi_bins + 1].
 *   - zeta.  Neighbour j of the list is bonded when r2_ij < r_hb r_hb and i donates to j or j to i
 *     through either hydrogen: the test of "Local order" with (r_hb, cos_hb), bit for bit.
 *     zeta_i = rho of the nearest listed neighbour that is not bonded - rho of the farthest bonded
 *     one.  Undefined without a bonded neighbour, or when every listed neighbour is bonded.  Bin
 *     (int)floor((zeta - zeta_lo) zeta_scale) clamped to 0 .. zeta_bins - 1, zeta_scale = zeta_bins /
 *     (zeta_hi - zeta_lo); undefined: slot zeta_bins of zeta_hist [zeta_bins + 1].
 *   - O-O-O angles.  Every unordered pair (j, k) of listed neighbours with both r2 < r_ang r_ang, j
 *     before k in the list: c = ((dj_x dk_x + dj_y dk_y) + dj_z dk_z) / sqrt(r2_j r2_k); bin
 *     (int)floor((c + 1.0) ang_scale) clamped to 0 .. ang_bins - 1, ang_scale = ang_bins / 2.0; a c
 *     that is not finite (a coincident oxygen): slot ang_bins of ang_hist [ang_bins + 1].  The
 *     histogram is in cos(theta) (observables.ooo_angle_distribution converts).
 *   - Outputs, all overwritten.  Each may be NULL, but not all five of rank_hist, lsi_hist, ang_hist,
 *     zeta_hist and sums; a histogram that is NULL costs no counters.  The four histograms are
 *     [R][...] with per_replica.  flagged [R].  sums [R][4] = (sum of the replica's defined I, their
 *     number, sum of its defined zeta, their number), the numbers as doubles, each sum in the order
 *     of "Local order"'s q_sum: bitwise reproducible, independent of the launch.  count_out [R][N] =
 *     m_i; nbr_out [R][N][MMC_SHELL_NBR] = the first 16 of the list, 0-based, then -1; lsi_out and
 *     zeta_out [R][N], NaN where undefined.  Nothing depends on the grid or option "wave_wgs".
 *   - Use (observables.py): neighbour_distance_distributions, lsi_distribution, zeta_distribution,
 *     ooo_angle_distribution, lsi_mean, zeta_mean.
 * Both box modes and either Coulomb style, records or arrays: the call reads coordinates only, and is
 * read-only exactly as mmc_batch_local_order is, with its preconditions (MMC_ERR_STATE).
 * MMC_ERR_ARG, checked before the batch: r_list not finite or <= 0; r_lsi, r_ang or r_hb outside
 * (0, r_list]; cos_hb outside (0, 1]; n_rank outside 1..MMC_SHELL_MAX_RANK; r_bins, lsi_bins,
 * ang_bins or zeta_bins outside 1..MMC_SHELL_MAX_BINS; lsi_max not finite or <= 0; zeta_lo >= zeta_hi
 * or either not finite; the five outputs above all NULL; and the bins of the histograms asked for
 * together, 1 + n_rank (r_bins + 1) + (lsi_bins + 1) + (ang_bins + 1) + (zeta_bins + 1) counting
 * only those that are not NULL, above MMC_SHELL_MAX_WORDS (a workgroup's 32-bit counters and a
 * wave's list, 4 bytes a word and 768 bytes, stay within 32 KiB of LDS).  Checked with the batch: r_list above
 * half of the smallest box.  Then the state; then MMC_ERR_UNSUPPORTED: fewer than 2 molecules or more
 * than 2^21.  On any error every output is left untouched. */
#define MMC_SHELL_CAP       64
#define MMC_SHELL_NBR       16
#define MMC_SHELL_MAX_RANK  16
#define MMC_SHELL_MAX_BINS  1024
#define MMC_SHELL_MAX_WORDS 8000
int32_t mmc_batch_shell_order(mmc_batch *b, double r_list, double r_lsi, double r_ang, double r_hb, double cos_hb,
    int32_t n_rank, int32_t r_bins, int32_t lsi_bins, double lsi_max, int32_t ang_bins,
    int32_t zeta_bins, double zeta_lo, double zeta_hi, int32_t per_replica,
    uint64_t *rank_hist, uint64_t *lsi_hist, uint64_t *ang_hist, uint64_t *zeta_hist, uint64_t *flagged,
    double *sums, int32_t *count_out, int32_t *nbr_out, double *lsi_out, double *zeta_out);

/* ---- Voronoi cells: volumes, asphericity and geometric neighbours of 3-site molecules ------------
 * The cutoff-free side of the local structure: the Voronoi cell of every oxygen of every replica in
 * one read-only pass -- its volume V (the local density of the two-state picture), its surface S, its
 * asphericity eta = S^3 / (36 pi V^2) (Ruocco, Sampoli and Vallauri, J. Chem. Phys. 96, 6167, 1992:
 * 2.25 in ice Ih and Ic, about 1.6 - 1.7 in the liquid), its faces (the geometric coordination number
 * and neighbour list) and the sums for <V> and <V^2> - <V>^2.  The reference has no such analysis; the
 * arithmetic is defined here, operation by operation, and restated in numpy by tests/voronoi_ref.py.
 * + - x / sqrt floor are correctly rounded fp64 and nothing is fused, so every output is reproducible
 * bit for bit.  Every dot product and every r^2 is (x x' + y y') + z z'; r_list r_list and the scales
 * named below are formed once, in fp64, by the host.
 *   - List.  The list of "Shell order" with the same r_list: neighbour k = 0 .. n - 1 of molecule i
 *     in rising (bits of rho_k^2, j), d_k = d(O_i, O_j) the signed image and rho_k^2 its r^2.  More
 *     than MMC_VORONOI_CAP = 64 in range: flag bit 0 (CAP), nothing else is done.  n = 0, or
 *     rho_0^2 = 0 (a coincident oxygen has no bisector plane): flag bit 1 (OPEN), nothing else is done.
 *     Two LISTED neighbours that coincide with each other are not looked for: they own bit-equal
 *     planes, each face is clipped by the other's plane with e(p) of rounding size and either sign,
 *     so one or both faces may vanish while the cell stays certified, its V short of that face's
 *     A rho / 6.  The outputs are still the ones this arithmetic defines, bit for bit; they are not
 *     the cell of the distinct sites.  Coincident oxygens do not occur in a chain (the overlap test).
 *   - Face k lies in the plane x . d_k = rho_k^2 / 2 around m_k = 0.5 d_k.  Its in-plane basis: with
 *     a the axis of the smallest |component| of d_k (the first of equal ones), w = d_k x e_a written
 *     out -- a = x: (0, d_z, -d_y); a = y: (-d_z, 0, d_x); a = z: (d_y, -d_x, 0) -- u = w / sqrt(w . w)
 *     (three divisions), q = d_k x u = (d_y u_z - d_z u_y, d_z u_x - d_x u_z, d_x u_y - d_y u_x),
 *     v = q / sqrt(q . q).  A point of the plane is x = m_k + s u + t v, and |x|^2 is taken as
 *     0.25 rho_k^2 + (s s + t t).
 *   - Polygon.  Face k starts as the vertices (s, t) = (-r, -r), (r, -r), (r, r), (-r, r), r = r_list,
 *     and is clipped by the planes m = 0, 1, ..., n - 1, m != k, in that order: a = u . d_m,
 *     b = v . d_m, c = 0.5 rho_m^2 - m_k . d_m; e(p) = (a s_p + b t_p) - c; p is inside when
 *     e(p) <= 0.  One clip makes a new vertex list from the old one p_0 .. p_(N-1): for j = 0 .. N - 1
 *     with q = p_(j+1), or p_0 after the last: if p_j is inside, p_j is appended; then, if exactly one
 *     of p_j and q is inside (a cut edge), w = e(p_j) / (e(p_j) - e(q)) and the vertex
 *     (s_p + w (s_q - s_p), t_p + w (t_q - t_p)) is appended.  A list that ends with fewer than three
 *     vertices is no face: the lane is done.  An append to a list that holds MMC_VORONOI_MAXV = 16
 *     vertices, or a third cut edge in one clip (rounding made the polygon non-convex), sets flag bit
 *     2 (POLY) and ends the face.  (With at most two cut edges the new list is never longer than
 *     j + 2 once p_j has been handled: a clip can be made in place.)  The largest polygon met on
 *     water and on lattices had 13 vertices.
 *   - Pruning.  g = the largest s s + t t of the face's current vertices.  Before plane m is applied,
 *     a face stops for good when 0.25 rho_m^2 > (0.25 rho_k^2 + g) MMC_VORONOI_PRUNE, PRUNE = 1 + 2^-20:
 *     a plane cuts a vertex x only if |x| > rho_m / 2, the ranks are in rising rho, and the margin is
 *     10^9 times the rounding of e(p), so neither this nor any later plane changes the list.  The
 *     rule changes no bit (option "voronoi_prune" = 0 walks every plane; tests compare the two).
 *   - Cell.  A_k = 0.5 |sum over j of (s_j t_(j+1) - s_(j+1) t_j)|, the sum from zero in rising j with
 *     p_N = p_0; 0 for no face.  S = sum of A_k, T = sum of A_k rho_k (rho_k = sqrt(rho_k^2)), each
 *     from zero in rising k; V = T / 6.0; eta = ((S S) S) / ((K V) V), K = 36.0 x 3.141592653589793.
 *     Face k is COUNTED when A_k > area_min: it is a geometric neighbour.  Every face enters S and V.
 *     (On perfect lattices rounding leaves faces of area ~ 1e-15 between second neighbours: area_min =
 *     1e-6 A^2 gives the textbook 6, 14, 12 and 16 faces of sc, bcc, fcc and diamond.)
 *   - Closure.  The cell is certified when a face is left and 4.0 (0.25 rho_k^2 + g_k) <= r_list r_list
 *     for every face left: an oxygen that could cut off a vertex at |x| lies within 2 |x| of O_i,
 *     and the list is complete to r_list.  Otherwise flag bit 1 (OPEN).  POLY and OPEN may both be set.
 *   - A molecule with a flag bit set enters no histogram and no sum.  Others add: vol_hist [v_bins +
 *     1] at (int)floor(V v_scale) clamped to 0 .. v_bins, v_scale = v_bins / v_max (last slot:
 *     beyond v_max); eta_hist [eta_bins + 1] at (int)floor((eta - 1.0) eta_scale) clamped to 0 ..
 *     eta_bins, eta_scale = eta_bins / (eta_max - 1.0), a value that is not finite to the last slot;
 *     face_hist [65] at the number of counted faces; per counted face side_hist [MMC_VORONOI_MAXV + 1]
 *     at its number of vertices and nbr_hist [r_bins + 1] at (int)floor(rho_k inv_dr) clamped to 0 ..
 *     r_bins, inv_dr = r_bins / r_list (the geometric-neighbour part of g_OO).
 *   - Outputs, all overwritten, each may be NULL but not all.  The five histograms are [R][...] with
 *     per_replica.  flagged [R][3]: molecules per flag bit (CAP, OPEN, POLY).  sums [R][8] = (number
 *     summed, sum V, sum V V, sum S, sum eta, sum of counted faces, sum of counted-face area, 0) over
 *     the replica's unflagged molecules in the order of "Local order"'s q_sum (lane l the molecules
 *     l, l + 64, ...; the lane sums in wave_sum_rows' order): bitwise reproducible, independent of the
 *     launch.  vol_out, area_out [R][N]: V and S, NaN where flagged; faces_out [R][N]: counted faces,
 *     or minus the flag bits; nbr_out [R][N][64]: the molecules (0-based) of the counted faces in
 *     rising rank, then -1; face_area_out [R][N][64]: their areas, then 0.  Nothing depends on the
 *     grid or on options "wave_wgs", "local_stage" and "voronoi_prune".
 *   - Use (observables.py): voronoi_volume_distribution, asphericity_distribution,
 *     voronoi_coordination, face_side_fractions, voronoi_neighbour_gr, voronoi_means,
 *     volume_fluctuation.
 *   - Limits.  64 neighbours reach to about 7.7 A at 1 g/cm^3, and a cell whose farthest vertex lies
 *     beyond r_list / 2 is OPEN and left out.  At low density (NIST configuration 4, 0.83 g/cm^3:
 *     3.5 % at r_list = 7.5 A) the cells left out are the largest, so the high-V tail and <V> are
 *     biased low; flagged says by how much.  r_list is bounded by half the smallest box: beyond it
 *     the minimum image is not the only image that can cut a cell.
 * Both box modes and either Coulomb style, records or arrays: the call reads O positions only, and is
 * read-only exactly as mmc_batch_shell_order is, with its preconditions (MMC_ERR_STATE).
 * MMC_ERR_ARG, checked before the batch: r_list or v_max not finite or <= 0; area_min not finite or
 * < 0; eta_max not finite or <= 1; v_bins, eta_bins or r_bins outside 1..MMC_VORONOI_MAX_BINS (which
 * keeps a workgroup's 32-bit counters, at most 3157 words, beside its waves' lists and polygons in
 * LDS); every output NULL.  Checked with the batch: r_list above half of the smallest box.  Then the
 * state; then MMC_ERR_UNSUPPORTED: fewer than 2 molecules or more than 2^21.  On any error every
 * output is left untouched. */
#define MMC_VORONOI_CAP      64
#define MMC_VORONOI_MAXV     16
#define MMC_VORONOI_MAX_BINS 1024
int32_t mmc_batch_voronoi(mmc_batch *b, double r_list, double area_min, int32_t v_bins, double v_max,
    int32_t eta_bins, double eta_max, int32_t r_bins, int32_t per_replica,
    uint64_t *vol_hist, uint64_t *eta_hist, uint64_t *face_hist, uint64_t *side_hist, uint64_t *nbr_hist,
    uint64_t *flagged, double *sums,
    double *vol_out, double *area_out, int32_t *faces_out, int32_t *nbr_out, double *face_area_out);

/* ---- Bond order: Steinhardt q_l, bond correlations, solid-like molecules and their clusters -----
 * Is there ice in the box, how much, and how large is the largest crystalline nucleus: Steinhardt's
 * bond-orientational order q_l (Steinhardt, Nelson and Ronchetti, Phys. Rev. B 28, 784, 1983), the
 * neighbour-averaged qbar_l (Lechner and Dellago, J. Chem. Phys. 129, 114707, 2008), the bond
 * correlations c_ij that ten Wolde, Ruiz-Montero and Frenkel (J. Chem. Phys. 104, 9932, 1996) and
 * CHILL+ (Nguyen and Molinero, J. Phys. Chem. B 119, 9369, 2015) classify molecules with, and the
 * clusters of solid-like molecules, for every molecule of every replica in one read-only pass over
 * the O-O neighbours (slot 0 of a molecule is "O").  The reference has no such analysis; the
 * arithmetic is defined here, operation by operation, and restated in numpy by
 * tests/bond_order_ref.py.  + - x / sqrt floor are correctly rounded fp64 and nothing is fused, so
 * every output is reproducible bit for bit.  No trigonometric function is used.
 *   d(x, y) is vector1D as in "Local order", per component, with the replica's own box.  Every r^2
 *   is (x x + y y) + z z.
 *   - Neighbours.  For molecule i: d_ij = d(O_i, O_j), r2_ij its r^2.  In range: every j != i with
 *     r2_ij < r_nb r_nb (the square formed by the host), ascending under the key (bit pattern of
 *     r2_ij, then j) -- the list of "Shell order" with r_list = r_nb.  count_i is their number and
 *     nb(i) the first n_i = min(count_i, n_nb) of them, j_1 .. j_n in that order ("rank order").  A
 *     molecule with count_i > n_nb is counted in TRUNCATED and processed like any other.  A molecule
 *     with count_i > MMC_SHELL_CAP = 64 is FLAGGED: it has no nb(i), no q_lm and no bonds of its
 *     own, and is not counted in truncated.
 *   - Bond vectors.  rho_k = sqrt(r2_k) and u_k = (d_x / rho_k, d_y / rho_k, d_z / rho_k) of
 *     neighbour k.  A molecule that is not flagged and has n_i = 0 or some rho_k = 0 is UNDEFINED;
 *     every other molecule that is not flagged is DEFINED.
 *   - Constants, formed once by the host in fp64, l in {3, 4, 6}: PI = 3.141592653589793;
 *     F_m = (l - m + 1)(l - m + 2) ... (l + m), an exact integer (F_0 = 1);
 *     N_m = sqrt(((2 l + 1) / (4 PI)) / F_m);  K = (4 PI) / (2 l + 1).
 *   - Harmonics of u = (x, y, z), m = 0 .. l, without the Condon-Shortley sign (it cancels in every
 *     output; negative m follow from conjugation and enter through the weights w_m):
 *       c_0 = 1, s_0 = 0;  c_m = x c_(m-1) - y s_(m-1);  s_m = x s_(m-1) + y c_(m-1)
 *       (the real and imaginary part of (x + i y)^m; each two products, then one sum);
 *       T_m^m = 1 3 5 ... (2 m - 1), exact (T_0^0 = 1);  T_(m+1)^m = ((2 m + 1) z) T_m^m;
 *       T_n^m = ((((2 n - 1) z) T_(n-1)^m) - ((n + m - 1) T_(n-2)^m)) / (n - m), n = m + 2 .. l
 *       (the m-th derivative of the Legendre polynomial P_n);
 *       A = N_m T_l^m;  Re Y_lm = A c_m;  Im Y_lm = A s_m.
 *   - Per molecule.  Re q_lm(i) = (Re Y_lm(u_1) + Re Y_lm(u_2) + ...) / n_i, the sum one term at a
 *     time in rank order, n_i as a double; Im q_lm likewise.  t_m = Re q_lm Re q_lm + Im q_lm Im q_lm;
 *     Q_i = t_0 + 2 t_1 + 2 t_2 + ... in rising m (w_0 = 1, w_m = 2);  q_l(i) = sqrt(K Q_i).
 *   - Per directed bond (i, j in nb(i)).  t_m = Re q_lm(i) Re q_lm(j) + Im q_lm(i) Im q_lm(j);
 *     D = t_0 + 2 t_1 + ... in rising m;  c_ij = D / (sqrt(Q_i) sqrt(Q_j)).  The bond is undefined
 *     when i or j is not defined, when Q_i or Q_j is 0, or when c_ij is not finite.
 *   - Averaged.  Re qbar_lm(i) = (Re q_lm(i) + Re q_lm(j_1) + Re q_lm(j_2) + ...) / (n_i + 1), in
 *     rank order; Im likewise; Qbar_i and qbar_l(i) from qbar_lm as Q_i and q_l(i) from q_lm.
 *     qbar_l(i) is undefined unless i and every molecule of nb(i) are defined.
 *   - Windows.  A defined bond is in A when a_lo <= c_ij <= a_hi and in B when b_lo <= c_ij <= b_hi
 *     (it may be in both); a_lo and b_lo may be -inf, a_hi and b_hi +inf.  n_A(i) and n_B(i) count
 *     the bonds of i in each.  CHILL+: l = 3, n_nb = 4, r_nb = 3.5 A, A = staggered (-inf, -0.8],
 *     B = eclipsed [-0.35, 0.25].
 *   - Solid-like.  i is defined, n_A(i) >= min_a and n_A(i) + n_B(i) >= min_ab.  (3, 4) with the
 *     CHILL+ windows selects cubic and hexagonal ice; a ten Wolde-Frenkel criterion is l = 6,
 *     n_nb = 16, A = [0.5, 1], min_a = 7, min_ab = 0.)
 *   - Clusters.  An undirected edge joins i and j when both are solid-like and j is in nb(i) or i in
 *     nb(j); clusters are the connected components, a solid-like molecule without edges a cluster
 *     of 1.  The label of a solid-like molecule is the lowest index of its cluster.
 *   - Bins: (int)floor(v scale) clamped to 0 .. bins - 1, the clamps made on the double, as "Shell
 *     order": q_l and qbar_l with v = q, scale = (double)q_bins over [0, 1]; c_ij with v = c + 1.0,
 *     scale = c_bins / 2.0 over [-1, 1].
 *   - Outputs, all overwritten, each may be NULL (but not all of them) and a NULL one costs nothing:
 *     a call that asks for q_hist, q_out and nbr_out only runs the neighbour phase alone, one
 *     without size_hist, stats and label_out has no cluster phase.  The histograms are [R][...] with
 *     per_replica.
 *     q_hist, qbar_hist uint64 [q_bins + 1]: molecules; last slot: q_l (qbar_l) undefined, flagged
 *       molecules included.
 *     c_hist uint64 [c_bins + 1]: directed bonds (i, j in nb(i)); last slot: undefined bonds.
 *     ab_hist uint64 [17][17]: the defined molecules at [n_A][n_B].
 *     size_hist uint64 [N + 1]: entry s = the number of clusters of s molecules.
 *     stats int64 [R][MMC_BO_STATS]: 0 defined, 1 undefined, 2 flagged, 3 truncated, 4 solid-like
 *       molecules, 5 clusters, 6 the largest cluster, 7 the sum of s^2 over the clusters.
 *     sums double [R][4] = (sum of the replica's defined q_l, their number, sum of its defined
 *       qbar_l, their number), in the order of "Local order"'s q_sum: bitwise reproducible.
 *     q_out, qbar_out double [R][N], NaN where undefined.  nbr_out int32 [R][N][MMC_BO_MAX_NB]:
 *       nb(i) by rank, then -1.  ab_out uint8 [R][N][2] = (n_A, n_B).  label_out int32 [R][N], -1
 *       where not solid-like.
 *     Nothing depends on the grid, on options "wave_wgs", "local_stage" and "bond_chunk", or on any
 *     order of lanes, waves or atomics.
 *   - Scratch.  q_lm travels between the phases in device scratch (197 bytes per molecule), so the
 *     replicas are worked off in chunks under a fixed budget (256 MiB), the phases of a chunk
 *     launched one after the other on the batch's stream.  Option "bond_chunk" = n > 0 sets the
 *     replicas per chunk (for tests of a ragged last chunk); 0 = by the budget.
 *   - Use (observables.py): steinhardt_distribution, bond_correlation_distribution, solid_fraction,
 *     largest_nucleus, nucleus_size_distribution, chill_plus_classes.
 * Both box modes and either Coulomb style, records or arrays: the call reads coordinates only, and is
 * read-only exactly as mmc_batch_local_order is, with its preconditions (MMC_ERR_STATE).
 * MMC_ERR_ARG, checked before the batch: l not 3, 4 or 6; n_nb outside 1..MMC_BO_MAX_NB; r_nb not
 * finite or <= 0; q_bins or c_bins outside 1..MMC_BO_MAX_BINS; a window bound that is NaN; every
 * output NULL.  Checked with the batch: r_nb above half of the smallest box.  Then the state; then
 * MMC_ERR_UNSUPPORTED: fewer than 2 molecules, or more than MMC_BO_MAX_MOL (the labels and sizes of a
 * replica's clusters, 8 bytes per molecule, stay in one workgroup's LDS).  On any error every output
 * is left untouched. */
#define MMC_BO_MAX_NB   16
#define MMC_BO_MAX_BINS 4096
#define MMC_BO_STATS    8
#define MMC_BO_MAX_MOL  8000
int32_t mmc_batch_bond_order(mmc_batch *b, int32_t l, double r_nb, int32_t n_nb, double a_lo, double a_hi,
    double b_lo, double b_hi, int32_t min_a, int32_t min_ab, int32_t q_bins, int32_t c_bins,
    int32_t per_replica, uint64_t *q_hist, uint64_t *qbar_hist, uint64_t *c_hist, uint64_t *ab_hist,
    uint64_t *size_hist, int64_t *stats, double *sums, double *q_out, double *qbar_out,
    int32_t *nbr_out, uint8_t *ab_out, int32_t *label_out);

/* ---- Cavities and occupancy: p_n(R), its moments and the cavity-size distribution ---------------
 * How many sites lie within R of a random point of the liquid, for up to eight radii at once, and
 * how far the nearest site is: the occupancy distribution p_n(R) of scaled-particle and
 * information theory (Hummer, Garde, Garcia, Pohorille and Pratt, PNAS 93, 8951, 1996).  p_0(R) is
 * the probability of a cavity of exclusion radius R, and -T ln p_0(R) the excess chemical potential
 * of a hard sphere that keeps the sites at R.  The reference has no such analysis; the arithmetic is
 * defined here and restated in numpy by tests/cavity_ref.py.  All results are integers or plain
 * copies: nothing is left to a tolerance.
 *   - Sites.  site = 0, 1 or 2: that atom slot of every molecule (slot 0 is the oxygen of every water
 *     deck here); site = -1: the stored centre of mass.  One site per molecule, N in all.
 *   - Probe points of mmc_batch_cavity.  Probe j of replica r is (u0, u1, u2) L_r: u0, u1 the two
 *     uniforms of Philox slot MMC_SLOT_CAVITY + 0, u2 the first uniform of slot MMC_SLOT_CAVITY + 1,
 *     counter draw0 + j, key = seed, replica index = the index in the batch; L_r the replica's own box
 *     with per-replica boxes.  MMC_SLOT_CAVITY == MMC_SLOT_WIDOM: this is bit for bit the COM that
 *     mmc_batch_widom draws for the same (seed, draw0 + j, r) (observables.widom_molecules;
 *     observables.cavity_points is the host mirror).  mmc_batch_cavity_at takes the caller's
 *     points_in [R][n_probe][3] instead.
 *   - Distances.  d = vector1D(point, site) (Ewald/boundaries.jl; csrc/mmc_device.hpp) per component
 *     with the replica's own box; r^2 = (dx dx + dy dy) + dz dz in unfused fp64.  (The kernel takes
 *     |d| through vector1D_abs: the same bits once squared.)
 *   - Occupancy.  For radius k, n_k = the number of sites with r^2 < radii[k] radii[k] (strict; the
 *     square formed in fp64 by the host).  occ_hist[k][min(n_k, n_cap)] += 1 per probe: [K][n_cap + 1],
 *     [R][K][n_cap + 1] with per_replica; the last bin means "n_cap or more".
 *     occ_mom[k] += (n_k, n_k n_k), unclamped, as 64-bit integers: [K][2] or [R][K][2].
 *     count_out [R][n_probe][K]: the unclamped n_k.
 *   - Nearest site.  The minimum over the sites under the key (bit pattern of r^2, then index j):
 *     ties go to the lower index.  nn_r2_out [R][n_probe] and nn_idx_out [R][n_probe] (0-based).
 *     Its histogram uses no square root: with dr = nn_max / nn_bins and e2[m] = (m dr)(m dr) for
 *     m = 0 .. nn_bins, both products in fp64, the bin is the largest m with e2[m] <= r^2 of the
 *     nearest site (numpy: searchsorted(e2, r2, side = "right") - 1).  nn_hist [nn_bins + 1], or
 *     [R][nn_bins + 1] with per_replica; the last bin means "at or beyond nn_max".  Summed from the
 *     top, nn_hist is p_0(R) at every edge m dr from one pass: the cavity-size distribution
 *     (observables.cavity_size_distribution).
 *   - Outputs.  All are overwritten, not accumulated.  Each may be NULL, but not all three of
 *     occ_hist, occ_mom and nn_hist; without nn_hist, nn_bins and nn_max are ignored.  All sums are
 *     integers: no order of lanes, waves, atomics or flushes can change a bit, whatever the grid or
 *     option "wave_wgs".
 *   - Use (observables.py): occupancy_probabilities, occupancy_moments, cavity_mu_ex,
 *     cavity_size_distribution, and information_theory_pn, the two-moment maximum-entropy p_n.
 * Both box modes and either Coulomb style: the call reads coordinates only -- no erfc table, no S(k)
 * -- and is read-only exactly as mmc_batch_local_order is (coordinates, S(k), flags, step counters
 * and random streams are not touched; S(k) need not be fresh).  Preconditions as
 * mmc_batch_rdf_sites: no proposals outstanding, no volume trial in flight, no run that failed
 * half-way (MMC_ERR_STATE).
 * MMC_ERR_ARG, checked before the batch: n_probe outside 1..2^20; site outside -1..2; n_radii outside
 * 1..MMC_CAVITY_MAX_RADII; radii NULL; a radius not finite, <= 0 or not strictly above the one before;
 * n_cap outside 1..MMC_CAVITY_MAX_CAP; with nn_hist, nn_bins outside 1..MMC_CAVITY_MAX_BINS or nn_max
 * not finite or <= 0; occ_hist, occ_mom and nn_hist all NULL; points_in NULL.  Checked with the
 * batch: a non-finite point; a radius above half of the smallest box; N^2 R n_probe >= 2^63 (the
 * moment sums could wrap).  Then the state; then MMC_ERR_UNSUPPORTED: more than 2^21 molecules.  On
 * any error every output is left untouched. */
#define MMC_SLOT_CAVITY        MMC_SLOT_WIDOM   /* the probe points ARE Widom's COM draws */
#define MMC_CAVITY_MAX_RADII   8
#define MMC_CAVITY_MAX_CAP     255
#define MMC_CAVITY_MAX_BINS    4096
int32_t mmc_batch_cavity(mmc_batch *b, int64_t n_probe, uint64_t seed, int64_t draw0, int32_t site,
                         int32_t n_radii, const double *radii, int32_t n_cap,
                         int32_t nn_bins, double nn_max, int32_t per_replica,
                         uint64_t *occ_hist, uint64_t *occ_mom, uint64_t *nn_hist,
                         double *points_out, int32_t *count_out, double *nn_r2_out, int32_t *nn_idx_out);
int32_t mmc_batch_cavity_at(mmc_batch *b, int64_t n_probe, const double *points_in, int32_t site,
                            int32_t n_radii, const double *radii, int32_t n_cap,
                            int32_t nn_bins, double nn_max, int32_t per_replica,
                            uint64_t *occ_hist, uint64_t *occ_mom, uint64_t *nn_hist,
                            int32_t *count_out, double *nn_r2_out, int32_t *nn_idx_out);

/* ---- Virtual volume moves: the pressure of every replica in one read-only pass -----------------
 * The volume-perturbation estimator (Eppenga and Frenkel; Harismiadis, Vorholz and Panagiotopoulos)
 *   beta P = ln < (V'/V)^N exp(-beta dU) > / dV
 * with dU what the NPT move of this library (Ewald/volumeChange.jl:59-147) would see: the change of
 * potential(..., "ewald") under its own rescale.  n_scale test boxes (1..8) per call, all evaluated
 * from one load of every replica's coordinates; nothing in the batch is written.
 *   - Test box k: L_k = scale[k] L and kappa_k = alpha / L_k with alpha = kappa L of the batch
 *     (Ewald/main.jl:290-291, the rule of mmc_batch_run_npt).
 *   - Test configuration: k_rescale's arithmetic (volumeChange.jl:62-80) on a copy: per COM
 *     component new = old * f and d = new - old, every atom of the molecule atom + d, f = scale[k],
 *     unfused fp64.
 *   - Energy: U_k = potential(..., "ewald") (Ewald/energy.jl:946-1032) of that configuration in box
 *     L_k -- LJ (Ewald/energy.jl:209-290) and EwaldReal (Ewald/ewalds.jl:293-376) behind the COM gate
 *     with the minimum image of L_k and the erfc table of kappa_k, RecipLong (Ewald/ewalds.jl:538-604)
 *     with the k-vector weights of PrepareEwaldVariables at (kappa_k, L_k) (Ewald/ewalds.jl:45-103) over
 *     the batch's k list, EwaldSelf at kappa_k (Ewald/ewalds.jl:829-833) -- in four parts
 *     (LJ, real, recip, self), each in mmc_batch_potential_ewald's normalisation.
 *   - U_0: the same evaluation at f = 1 (L_0 = 1.0 L, kappa_0 = alpha / L_0), by the same kernels in
 *     the same call.
 *   - du_out[r][k][0..3] = (dLJ, dreal, drecip, dself), each part of U_k minus that part of U_0;
 *     base_out[r][0..3] = the four parts of U_0; dU = ((dLJ + dreal) + drecip) + dself.  A scale of
 *     exactly 1.0 gives four zeros and dU == 0.0 bit for bit.
 *   - Weight: w = exp(-dU / T + N ln(scale^3)), N the number of molecules, scale^3 = (s s) s: the
 *     acceptance test of volumeChange.jl:129-130 at P = 0.  boltz_sum[r][k] += w.
 *   - Order of summation.  A replica's pair terms are summed per tile pair (64 x 64 molecules, tiles
 *     I <= J in row-major order) by a fixed tree over the workgroup's 256 threads, the tile pairs then
 *     in index order; S(k) per (kx, ky) column lane l adding atoms l, l + 64, ... and the 64 lanes by
 *     a fixed tree; the reciprocal energy thread t adding k = t, t + 1024, ..., lanes by the same
 *     tree, the 16 waves in index order.  Parts, differences, exp and the accumulation are the
 *     host's, in fp64, replica by replica, k = 0 .. n_scale - 1.  None of it depends on the grid or on
 *     option "wave_wgs": results are bitwise reproducible.
 *   - Overlap: an atom pair with r^2 < 0.5 and opposite charges inside the COM gate (ewalds.jl:359),
 *     as mmc_batch_potential_ewald reports it with per-replica boxes.  A replica that overlaps at
 *     test box k, or whose dU is not finite, has weight 0 there and n_overlap[r][k] += 1; an overlap
 *     at f = 1 does so for every k of the replica.  Where an overlap decides, the real part reported
 *     (du_out[r][k][1], base_out[r][1]) is +inf, as that call's energy is.
 *   - Read-only: coordinates, S(k), cfac and tables of the batch, flags, step counters and random
 *     streams are not touched; a chain with these calls interleaved is bit-identical to one without.
 *     S(k) need not be fresh.
 * MMC_ERR_STATE as mmc_batch_potential_ewald: proposals outstanding, a volume trial in flight.
 * MMC_ERR_ARG: n_scale outside 1..8; scale NULL; a scale not finite or <= 0; L_k < 2 r_cut;
 * temperature <= 0 or not finite; all four outputs NULL.  MMC_ERR_UNSUPPORTED, nothing computed:
 * per-replica boxes (mmc_batch_set_boxes); Wolf style; a system the table kernels refuse (not
 * identical 3-atom molecules); (kappa_k, r_cut) outside the erfc table's domain at the smallest L_k
 * (kappa <= 0.5 and kappa sqrt(r_cut^2 + 100) <= 4); a replica whose atoms' phases do not fit one
 * workgroup's LDS (56 bytes per atom: about 2800 atoms).  On any error every output is untouched. */
/* (`temperature` is this call's own argument: the batch's per-replica temperatures,
 * mmc_batch_set_temperatures, are not read) */
int32_t mmc_batch_volume_perturb(mmc_batch *b, int32_t n_scale, const double *scale /* [K] */,
                                 double temperature,
                                 double *boltz_sum  /* [R][K] in/out, may be NULL */,
                                 int64_t *n_overlap /* [R][K] in/out, may be NULL */,
                                 double *du_out     /* [R][K][4] may be NULL */,
                                 double *base_out   /* [R][4]    may be NULL */);

/* ---- Save and resume: bulk state records ------------------------------------------------------------
 * Everything of a replica that the chains carry from one call to the next, as one fixed-size
 * RECORD per replica, moved in bulk; and one mmc_state_info that describes the batch the records
 * belong to.  The library moves records and checks that the receiving batch is ALREADY configured
 * for them; configuring a fresh batch (mmc_batch_set_coulomb_style, _set_boxes, _set_temperatures,
 * _set_orientations, _volume_change, _set_solute) and the file are the caller's (checkpoint.py,
 * Batch.save / Batch.load).  No entry point here decides, proposes or evaluates a move.
 *
 * Guarantee: after mmc_batch_set_state of all R replicas into a batch of the same system, created
 * from ANY coordinates and brought into the saved mode, every chain continues bit for bit (same
 * energies, decisions, coordinates and S(k)) provided the resuming batch uses the same options
 * `kernel`, parts, `persistent` / `server_wgs`, `steps_per_launch` and `half_k` -- the condition
 * mmc_run_params::replica0 documents for shardings.  Options are not part of the state: the caller
 * sets them, as at creation.  The caller also keeps what the batch never held: the running
 * energies, the mmc_chain array, rung / attempt / accept and the exchange round, NPT statistics.
 *
 * mmc_state_info: 8-byte fields only, 42 of them (336 bytes).
 *   identity (a mismatch is MMC_ERR_ARG: these records are not of this batch's system)
 *     magic        MMC_STATE_MAGIC
 *     version      MMC_STATE_VERSION
 *     R            replicas of the batch that wrote the info
 *     n_mol        molecules per replica (3 atoms each)
 *     nkvecs       k-vectors the device holds: 293 with half_k, else 337
 *     half_k       1 / 0
 *     lj_rcut, qq_rcut
 *     topology     FNV-1a (64 bit) over n_types, atype, charge, eps, sig as given to mmc_batch_create
 *     nk, k_sq_max, factor
 *   mode (a difference from how the batch is configured NOW is MMC_ERR_STATE)
 *     coulomb_style, s_stale      mmc_batch_set_coulomb_style and whether S(k) awaits a rebuild
 *     per_box      1: per-replica boxes (mmc_batch_set_boxes); alpha is compared only then
 *     alpha
 *     temps_on     1: per-replica temperatures are set
 *     quat_mode    0 / 1 / 2 (mmc_batch_set_orientations); db[9] is compared only when not 0
 *     db[9]
 *     box, kappa   the shared box and kappa; compared only when per_box == 0
 *   batch-level scalars (applied by mmc_batch_set_state)
 *     steps_done   position of the random streams ("Random streams")
 *     r_mol_max    bound on an atom's distance from its centre of mass (+inf: unknown)
 *     rigid_only   1: every committed move was drawn on the device
 *   the fixed solute (mode: a difference is MMC_ERR_STATE)
 *     solute_on    1: a solute is set (mmc_batch_set_solute); 0: none
 *     solute_hash  FNV-1a (64 bit) over n_sites (8 bytes) and mol, charge, eps, sig as given to
 *                  mmc_batch_set_solute; 0 without a solute
 *     reserved[8]  zero
 * Of the receiving batch, R may differ from info->R (a record range of another batch); everything
 * else of the identity must agree. */
#define MMC_STATE_MAGIC 0x31544154534d434dULL /* "MCMSTAT1" */
#define MMC_STATE_VERSION 1
typedef struct {
    uint64_t magic;
    int64_t version;
    int64_t R, n_mol, nkvecs, half_k;
    double lj_rcut, qq_rcut;
    uint64_t topology;
    int64_t nk, k_sq_max;
    double factor;
    int64_t coulomb_style, s_stale, per_box;
    double alpha;
    int64_t temps_on, quat_mode;
    double db[9];
    double box, kappa;
    int64_t steps_done;
    double r_mol_max;
    int64_t rigid_only;
    int64_t solute_on;
    uint64_t solute_hash;
    int64_t reserved[8];
} mmc_state_info;

/* The record of one replica, the single definition of the format (a pure host function: no device,
 * no batch; it reads n_mol, nkvecs and quat_mode of `info`).  offsets[0..7], in bytes from the
 * start of the record, every one a multiple of 8 and [3] .. [7] of 16:
 *   [0] box          double: the replica's box (the shared box when per_box == 0)
 *   [1] temperature  double: 0.0 when temps_on == 0
 *   [2] flags        uint64: bit 0 per_box, bit 1 temps_on, bit 2 quat_mode != 0 (then 8 zero bytes)
 *   [3] com          double [n_mol][3]      as mmc_batch_get_replica returns it
 *   [4] coords       double [3 n_mol][3]    as mmc_batch_get_replica returns it
 *   [5] S            double [nkvecs][2]     the buffer that is sumQExpOld, in DEVICE order (the
 *                    order of mmc_get_kvectors of a batch with this half_k), bit for bit: the
 *                    incrementally updated S(k), not a fresh sum
 *   [6] quat         double [n_mol][4]      only when quat_mode != 0 (else [6] == [7])
 *   [7] end of the data
 * Sections are padded to 16 bytes and the record to *record_bytes, a multiple of 64; padding is 0.
 * `info` points to an mmc_state_info (void * here and below: the Julia binding passes a Ref). */
int32_t mmc_state_record_layout(const void *info, int64_t *offsets /* [8] */, int64_t *record_bytes);
/* The info of the batch as it is configured now. */
int32_t mmc_batch_state_info(mmc_batch *b, void *info /* mmc_state_info, out */);
/* Pack replicas [r0, r0 + nr) on the device (k_state_pack) and deliver them to `records`, host
 * memory of nr * record_bytes.  Changes nothing.  MMC_ERR_STATE while proposals are outstanding
 * (mmc_batch_eval without mmc_batch_settle) or a volume trial is open.  Works in chunks of option
 * "state_chunk" replicas (0: by a budget of 256 MiB of staging) through two pinned buffers: the
 * pack of one chunk runs while the other is copied out.  Option "state_delivery": 1 = the kernels
 * write and read the mapped pinned buffers themselves, 0 = device memory and a copy, -1 (default) =
 * what measured faster for each call: 1 for mmc_batch_get_state, 0 for mmc_batch_set_state. */
int32_t mmc_batch_get_state(mmc_batch *b, int64_t r0, int64_t nr, void *records);
/* Validate `info` against the batch (identity: MMC_ERR_ARG; mode: MMC_ERR_STATE; a record whose
 * box or temperature the batch's setters would refuse: MMC_ERR_ARG) -- nothing is changed on any
 * refusal -- then unpack the records into replicas [r0, r0 + nr) (k_state_unpack): the SoA arrays,
 * the per-molecule records and fixed-point centres of mass of homogeneous systems (with the
 * replica's own box), the orientations; S(k) into BOTH buffers with buffer 0 current, the state
 * mmc_batch_recip_long leaves; with per-replica boxes the box, kappa = alpha / box and the cfac row
 * and erfc table of exactly these replicas; the temperature.  Applies the batch-level scalars
 * (r_mol_max and rigid_only exactly when the range is the whole batch, else their weaker
 * combination), marks the candidate lists and the host mirror stale, and after a failed run makes
 * the batch usable again once every replica has been set.  Other replicas keep every bit. */
int32_t mmc_batch_set_state(mmc_batch *b, const void *info /* mmc_state_info */, int64_t r0, int64_t nr,
                            const void *records);

/* ---- the one collective of a sharded run: RCCL over xGMI ---------------------
 * Replicas shard over GPUs with no data-path collective; what is reduced, once per block, is a
 * handful of observables (sums of energies and acceptance counters, the maximum of the elapsed
 * time).  For hosts without torch (the reference's language is Julia): one process per GPU,
 *   rank 0:    mmc_dist_unique_id(id), then id goes to the other ranks by whatever the host has (a
 *              file, a socket, MPI);
 *   all ranks: mmc_dist_init(rank, world, id, device, &d)      -- ncclCommInitRank, collective;
 *              mmc_dist_reduce(d, sums, n_sum, maxima, n_max)  -- in place: two ncclAllReduce
 *              (ncclSum / ncclMax, fp64) on the communicator's own stream;
 *              mmc_dist_destroy(d).
 * librccl.so is loaded at the first of these calls (MMC_ERR_UNSUPPORTED if it is not there); the
 * library itself links libamdhip64 only. */
typedef struct mmc_dist mmc_dist;
int32_t mmc_dist_unique_id(uint8_t id[128]);
int32_t mmc_dist_init(int32_t rank, int32_t world, const uint8_t id[128], int32_t device,
                      mmc_dist **out);
int32_t mmc_dist_reduce(mmc_dist *d, double *sums, int64_t n_sum, double *maxima, int64_t n_max);
int32_t mmc_dist_destroy(mmc_dist *d);

#ifdef __cplusplus
}
#endif
#endif
