// mmc_deletion.hpp -- k_deletion_wave: the deletion (binding) energy of existing molecules on the
// wave-per-unit scheme of k_move_eval_wave (mmc_wave.hpp), one wavefront per (replica, molecule);
// the mirror image of k_widom_wave (mmc_widom.hpp).
//
// The reference has no deletion code; the deletion energy is defined through its own total energy
// (include/mmc_hip.h, mmc_batch_deletion): what potential(..., "ewald") (Ewald/energy.jl:946-1032)
// loses when molecule i of the committed configuration is taken out,
//   dU = LJ_poly_dU(i)                         energy.jl:209-290
//      + EwaldShort(i)                         ewalds.jl:892-910 -> EwaldReal :293-376
//      + factor sum_k cfac_k (2 Re(conj(S_k) s_k) - |s_k|^2)     RecipLong(N) - RecipLong(N \ i), :538-604
//      - factor kappa / sqrt(pi) sum_a q_a^2   EwaldSelf(N) - EwaldSelf(N \ i), :829-833
// with S_k the committed structure factor (molecule i included) and s_k molecule i's own.
// A deletion is the one-state half of a trial move whose molecule is an existing one, so the unit is
// k_widom_wave's with the test molecule replaced by a record of the batch:
//   * molecule i's 96-byte record (one coalesced load of its 128-byte line) is the lane-distributed
//     register, placed in MoveRec layout in the proposal slot;
//   * the reciprocal part: the phase rows of its three atoms (phase_row_moderate, the reference's
//     recurrence), then lane per k over the half-space list against the replica's CURRENT S(k),
//     |S|^2 - |S - s|^2;
//   * the pair part is mmc_wave_unit.inc with one state (WV_NS = 1) and i0 = i: the scan lets the
//     molecule itself through and process() drops it;
//   * lane 0 combines the sums (mmc_combine_parts' arithmetic for one state) and stores the three
//     terms and the overlap flag.
// k_deletion_reduce (a wave per replica) then forms dU, the flags, the weights exp(+dU / T), the
// per-replica sums in a fixed order and the histogram of dU.
// Nothing the chains own is written: coordinates, S(k), flags and step counters are only read.
#pragma once
#include "mmc_widom.hpp"

#ifndef DELETION_OCC
#define DELETION_OCC 4 // waves per SIMD k_deletion_wave is compiled for (no scratch)
#endif

struct DeletionArgs {
    const int32_t *sel;  // [n] the selected molecules, 0-based (0, 1, .. N - 1 when the caller selects all)
    double *terms;       // [R][n][3]: d_lj, d_real, d_recip + self
    uint8_t *flags;      // [R][n]
    const uint8_t *scur; // [R] which S buffer holds the replica's committed S(k)
    int32_t n;           // selected molecules per replica
    double self_d;       // -factor kappa / sqrt(pi) sum_a q_a^2 (the host's arithmetic)
};

// grid: any number of workgroups of WV_WAVES waves; wave w of workgroup g takes units
// g * WV_WAVES + w, + gridDim.x * WV_WAVES, ... (k_move_eval_wave's map).  Unit u = entry u % n of
// replica u / n: a wave's consecutive units are consecutive molecules of one replica.  IMG: exactly
// k_move_eval_wave's condition (the molecule is one of the batch's own).
template <bool IMG>
__global__ __launch_bounds__(WV_WAVES * 64) __attribute__((amdgpu_waves_per_eu(DELETION_OCC, DELETION_OCC))) void k_deletion_wave(
    BatchView bv, const double *__restrict__ rec, const double *__restrict__ qq_tab,
    const int32_t *__restrict__ kpack, FastConsts fc, PairParams pp, DeletionArgs da, int n_units)
{
    UNIT_PROLOGUE();
    const double *const pvw = sm.pvw[wv]; // (unused: no pending commit)
    const int n_sel = da.n;

    UNIT_FOR(unit) {
        const int lane = unit_lane(lane0);
        const int r = unit / n_sel, ent = unit - r * n_sel;
        const int i0 = __builtin_amdgcn_readfirstlane(da.sel[ent]);
        const double *const myrec = rec + (int64_t)r * n_mol * MMC_RSTRIDE;

        const double mw = unit_load_record(myrec, i0, lane);
        const double w = unit_proposal_slot(mw, lane);

        // reciprocal part: s_k of molecule i0 against S_k (which holds it), cfac (|S|^2 - |S - s|^2)
        unit_recip_energy<-1>(sm, wv, bv, kpack, fc, r, da.scur[r], mw, lane, nkv, box);

        // ================= pair part: mmc_wave_unit.inc, one state, the molecule itself dropped =================
        const int pend = -1, scur = 0;
        const bool do_pairs = true, do_recip = false;
        const int j_begin = 0, j_end = n_mol;
        (void)scur; (void)pvw;
#define WV_NS 1
#define WV_SUBST 0
#define WV_IMG IMG
#define WV_UNIT_NO_STORE
#define WV_CQ_BASE (bv.comq + (int64_t)r * 3 * bv.cq_stride)
#include "mmc_wave_unit.inc"
#undef WV_CQ_BASE
#undef WV_UNIT_NO_STORE
#undef WV_IMG
#undef WV_SUBST
#undef WV_NS
        unit_store_terms(sm, wv, lane, bv.factor, da.self_d, da.terms + (int64_t)unit * 3, da.flags + unit);
    }
}

struct DeletionReduceArgs {
    const double *terms;      // [R][n][3]
    uint8_t *flags;           // [R][n]: the non-finite bit is added here
    double *esum;             // [R][4]: sum d_lj, sum d_real, sum d_recip, number summed
    double *boltz;            // [R] in / out
    long long *n_flag;        // [R] in / out
    unsigned long long *hist; // [n_bins + 2] or [R][n_bins + 2], zeroed by the host; or NULL
    double u_lo, u_hi, scale; // scale = n_bins / (u_hi - u_lo), the host's fp64
    double inv_temp;
    int32_t n, n_bins, per_replica, R;
};

// The slot of dU in a histogram of n_bins + 2 counters: 0 below u_lo, n_bins + 1 at or above u_hi
// (or where rounding lifts k to n_bins), else floor((dU - u_lo) * scale) + 1 -- unfused.  Host
// mirror: metropolismontecarlo_amd/observables.py energy_bins.
__device__ __forceinline__ int deletion_slot(double du, double u_lo, double u_hi, double scale, int n_bins)
{
    if (du < u_lo)
        return 0;
    if (du >= u_hi)
        return n_bins + 1;
    const double k = floor((du - u_lo) * scale);
    return k >= (double)n_bins ? n_bins + 1 : (int)k + 1;
}

// One wave per replica (workgroup g takes replicas g, g + gridDim.x, ...).  Lane l takes the
// replica's entries l, l + 64, ... in that order: dU = (d_lj + d_real) + d_recip, the flags, and for
// an unflagged entry the three terms, 1.0 and exp(+dU / T) added to the lane's five sums; then the 64
// lane sums by wave_sum_rows (DPP, fixed order), as k_dipoles: the bits do not depend on the launch.
// The bins are integer counters -- order-free: the summed form goes through 32-bit counters in LDS
// (a launch counts fewer than 2^31 entries) and one 64-bit atomic per touched bin and workgroup at
// the end, the per-replica form straight into the replica's row.
__global__ __launch_bounds__(64) void k_deletion_reduce(DeletionReduceArgs ra)
{
    extern __shared__ unsigned int lh[]; // [n_bins + 2] (the summed form only)
    const int lane = threadIdx.x;
    const int n = ra.n, slots = ra.n_bins + 2;
    const bool to_lds = ra.hist && !ra.per_replica;
    if (to_lds) {
        for (int q = lane; q < slots; q += 64)
            lh[q] = 0u;
        __syncthreads();
    }
    for (int r = blockIdx.x; r < ra.R; r += gridDim.x) {
        const double *t = ra.terms + (int64_t)r * n * 3;
        uint8_t *f = ra.flags + (int64_t)r * n;
        double a[5] = { 0.0, 0.0, 0.0, 0.0, 0.0 };
        double nf = 0.0; // flagged entries of this lane (exact: integers below 2^31)
        for (int e = lane; e < n; e += 64) {
            const double t0 = t[(int64_t)e * 3], t1 = t[(int64_t)e * 3 + 1], t2 = t[(int64_t)e * 3 + 2];
            const double du = (t0 + t1) + t2;
            const int fl = f[e] | (isfinite(du) ? 0 : MMC_WIDOM_NONFINITE);
            f[e] = (uint8_t)fl;
            if (fl) {
                nf += 1.0;
                continue;
            }
            a[0] += t0;
            a[1] += t1;
            a[2] += t2;
            a[3] += 1.0;
            a[4] += exp(du * ra.inv_temp);
            if (ra.hist) {
                const int s = deletion_slot(du, ra.u_lo, ra.u_hi, ra.scale, ra.n_bins);
                if (to_lds)
                    atomicAdd(&lh[s], 1u);
                else
                    atomicAdd(&ra.hist[(int64_t)r * slots + s], 1ULL);
            }
        }
        double s[5];
#pragma unroll
        for (int q = 0; q < 5; q++)
            s[q] = wave_sum_rows(a[q]);
        const double nfs = wave_sum_rows(nf);
        if (lane == 0) {
            if (ra.esum) {
#pragma unroll
                for (int q = 0; q < 4; q++)
                    ra.esum[4 * (int64_t)r + q] = s[q];
            }
            ra.boltz[r] = ra.boltz[r] + s[4]; // (added to the caller's value last)
            ra.n_flag[r] += (long long)nfs;
        }
    }
    if (to_lds) {
        __syncthreads();
        for (int q = lane; q < slots; q += 64) {
            const unsigned int v = lh[q];
            if (v)
                atomicAdd(&ra.hist[q], (unsigned long long)v);
        }
    }
}
