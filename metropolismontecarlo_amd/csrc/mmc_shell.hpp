// mmc_shell.hpp -- order between the first and second shell of 3-site molecules, read-only beside
// the chains:
//   k_shell_order_wave   per molecule: its O-O neighbours inside r_list sorted by distance (up to
//                        MMC_SHELL_CAP of them), and from that list the rank-resolved distance
//                        histograms, the local structure index, Russo and Tanaka's zeta and the
//                        O-O-O angles
// The arithmetic is stated in include/mmc_hip.h ("Shell order") and restated in numpy by
// tests/shell_order_ref.py; slot 0 of a molecule is the heavy atom, slots 1 and 2 the hydrogens.
// The per-replica sums are k_local_qsum's (mmc_local.hpp) over the per-molecule arrays.
//
// The scheme is mmc_nbr.hpp's: a persistent workgroup takes a contiguous run of the R N molecules
// (RunCursor), stages the O positions of every replica its run touches in LDS (STAGE), and its waves
// take the run's molecules of that replica in turn; inside a molecule a wave waits for nobody.
//
// One molecule i, one wave:
//   scan     scan_list: (bits of r^2, j) of the O inside r_list to the wave's list in LDS.  A pass
//            that would take the list beyond MMC_SHELL_CAP flags the molecule and ends its scan:
//            nothing is truncated.
//   sort     rank_sort: lane k then owns neighbour k, and the lanes hold the list in rising r^2 --
//            every radius selects a prefix of the lanes.
//   bonds    lanes with r^2 < r_hb^2 load their neighbour's nine coordinates and make
//            the four tests of the pair (HbPair; only where zeta is asked for).
//   reduce   rank bins by lanes < n_rank; LSI and zeta by lane reads and serial sums in rising k;
//            angles by an outer loop over j < m_ang with lanes k > j taking one cosine each.
// Counters: 32-bit, in LDS, one set per workgroup that its waves add to with LDS atomics, added to the
// 64-bit global ones whenever the workgroup leaves a replica -- integer adds, any order.  (A
// workgroup adds at most N x 2016 angles of one replica before that: below 2^32 for the 2^21
// molecules allowed.)  A set per wave, as k_local_order_wave keeps them, was measured first: with
// the default bins (2992 words) it left room for two waves per workgroup and three workgroups per
// compute unit, and the call took 2.2 times what it took with a tenth of the bins.
#pragma once
#include "mmc_local.hpp"

// MMC_SHELL_CAP (64 neighbours in a list: one lane each once sorted) and MMC_SHELL_NBR (16 of them in
// nbr_out) are include/mmc_hip.h's
static_assert(MMC_SHELL_CAP == NBR_CAP, "the list of scan_list: one lane per listed neighbour");

struct ShellArgs {
    const double *box_r;            // [R] per-replica boxes, or NULL: bv.box
    unsigned long long *flagged;    // [R], zeroed by the host
    unsigned long long *rank_hist;  // [n_rank][r_bins + 1] or [R][..], zeroed by the host; or NULL
    unsigned long long *lsi_hist;   // [lsi_bins + 1] or [R][..]; or NULL
    unsigned long long *ang_hist;   // [ang_bins + 1] or [R][..]; or NULL
    unsigned long long *zeta_hist;  // [zeta_bins + 1] or [R][..]; or NULL
    int32_t *count;                 // [R][N] or NULL
    int32_t *nbr;                   // [R][N][16] or NULL
    double *lsi_all, *zeta_all;     // [R][N] or NULL
    double rl2, rlsi2, rang2, rhb2, cos2;       // squares, formed by the host
    double inv_dr, lsi_scale, ang_scale, zeta_lo, zeta_scale;
    int32_t n_rank, r_bins, lsi_bins, ang_bins, zeta_bins;
    int32_t o_lsi, o_ang, o_zeta, hs; // the counter words: [0] flagged, [1, o_lsi) ranks, ..., hs in all
    int32_t per_replica, R;
};

// (int)floor(x) clamped to [0, top]; x finite or +-inf
__device__ __forceinline__ int sh_bin(double x, int top)
{
    return (int)fmin(fmax(floor(x), 0.0), (double)top);
}

// REC, STAGE, grid: as k_local_order_wave.
// dynamic LDS: [nw] lists of NBR_LIST_BYTES, [hs] counters, then (STAGE) 3 N doubles at the next
// multiple of 16 bytes.
template <bool REC, bool STAGE>
__global__ __launch_bounds__(NBR_WAVES * 64) void k_shell_order_wave(BatchView bv, const double *__restrict__ rec,
                                                                    ShellArgs sa)
{
    extern __shared__ __align__(16) unsigned char sh_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nw = (int)(blockDim.x >> 6);
    const int n_mol = bv.n_mol, hs = sa.hs;
    unsigned long long *const keys = reinterpret_cast<unsigned long long *>(sh_lds + (size_t)wv * NBR_LIST_BYTES);
    int *const idx = reinterpret_cast<int *>(keys + MMC_SHELL_CAP);
    unsigned *const hw = reinterpret_cast<unsigned *>(sh_lds + (size_t)nw * NBR_LIST_BYTES); // the workgroup's
    double *const pos = reinterpret_cast<double *>(
        sh_lds + (((size_t)nw * NBR_LIST_BYTES + 4 * (size_t)hs + 15) & ~(size_t)15));
    for (int q = tid; q < hs; q += (int)blockDim.x)
        hw[q] = 0u;
    __syncthreads();

    const bool want_lsi = sa.lsi_hist || sa.lsi_all, want_zeta = sa.zeta_hist || sa.zeta_all;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const Sites<REC, STAGE> sites{ bv, rec, pos };

    for (RunCursor rc(sa.R, n_mol); rc.next();) { // the run's molecules of one replica: [rc.lo, rc.hi) of replica r
        const int r = rc.r;
        if constexpr (STAGE)
            stage_sites(sites, r);
        const BoxConsts bc = box_consts(sa.box_r ? sa.box_r[r] : bv.box);

        for (int i = rc.lo + wv; i < rc.hi; i += nw) {
            const int64_t g = (int64_t)r * n_mol + i;
            double ci[9]; // the wave's molecule: wave-uniform
            load_sites9<REC>(bv, rec, r, i, ci); // O, H, H

            // ---- scan: the list, unsorted, in rising j
            int m;
            const bool over = !scan_list(sites, r, i, ci[0], ci[1], ci[2], bc, sa.rl2, keys, idx, lane, m);

            if (over) { // wave-uniform: in no histogram
                if (lane == 0) {
                    atomicAdd(&hw[0], 1u);
                    if (sa.count)
                        sa.count[g] = -1;
                    if (sa.lsi_all)
                        sa.lsi_all[g] = nan;
                    if (sa.zeta_all)
                        sa.zeta_all[g] = nan;
                }
                if (sa.nbr && lane < MMC_SHELL_NBR)
                    sa.nbr[MMC_SHELL_NBR * g + lane] = -1;
                continue;
            }

            // ---- sort: lane n's entry to slot rank(n); lane k then reads slot k
            const bool mine = lane < m;
            unsigned long long key;
            int jn;
            rank_sort(keys, idx, m, lane, key, jn);

            // lane k < m: neighbour k.  r^2 from the key; the signed image for the angles
            const double r2 = mine ? __longlong_as_double((long long)key) : 0.0;
            const double rho = sqrt(r2);
            double ox, oy, oz;
            sites.get(r, mine ? jn : i, ox, oy, oz);
            const double ex = vector1D(ci[0], ox, bc), ey = vector1D(ci[1], oy, bc), ez = vector1D(ci[2], oz, bc);

            // ---- rank histograms: lane k is rank k + 1
            if (sa.rank_hist && lane < sa.n_rank) {
                const int kb = mine ? sh_bin(rho * sa.inv_dr, sa.r_bins - 1) : sa.r_bins;
                atomicAdd(&hw[1 + lane * (sa.r_bins + 1) + kb], 1u); // a row per lane
            }

            // ---- LSI over the n neighbours inside r_lsi, neighbour n + 1 closing the last gap
            if (want_lsi) { // wave-uniform
                const int n = __popcll(wave_ballot(mine && r2 < sa.rlsi2)); // a prefix of the lanes
                double lsi = nan;
                if (n >= 1 && m >= n + 1) { // wave-uniform
                    const double delta = wave_pick(rho, min(lane + 1, 63)) - rho; // lanes < n: gap k + 1
                    double s = lane_f64(delta, 0);
                    for (int k = 1; k < n; k++)
                        s = s + lane_f64(delta, k);
                    const double mean = s / (double)n;
                    const double dev = (delta - mean) * (delta - mean);
                    double v = lane_f64(dev, 0);
                    for (int k = 1; k < n; k++)
                        v = v + lane_f64(dev, k);
                    lsi = v / (double)n;
                }
                if (lane == 0) {
                    if (sa.lsi_hist)
                        atomicAdd(&hw[sa.o_lsi + (n >= 1 && m >= n + 1 ? sh_bin(lsi * sa.lsi_scale, sa.lsi_bins - 1) : sa.lsi_bins)], 1u);
                    if (sa.lsi_all)
                        sa.lsi_all[g] = lsi;
                }
            }

            // ---- zeta: the nearest listed neighbour that is not bonded minus the farthest bonded one
            if (want_zeta) { // wave-uniform
                bool bonded = false;
                if (mine && r2 < sa.rhb2) {
                    double cj[9];
                    load_sites9<REC>(bv, rec, r, jn, cj);
                    double ui[2][3];
                    hb_arms(ci, bc, ui);
                    const HbPair hp(ci, ui, cj, bc);
                    bonded = hp.bonded(0, sa.cos2) || hp.bonded(1, sa.cos2) || hp.bonded(2, sa.cos2) || hp.bonded(3, sa.cos2);
                }
                const unsigned long long bm = wave_ballot(bonded), fm = wave_ballot(mine && !bonded);
                double zeta = nan;
                if (bm != 0ULL && fm != 0ULL) // wave-uniform
                    zeta = lane_f64(rho, __builtin_ctzll(fm)) - lane_f64(rho, 63 - __builtin_clzll(bm));
                if (lane == 0) {
                    if (sa.zeta_hist)
                        atomicAdd(&hw[sa.o_zeta + (bm != 0ULL && fm != 0ULL
                                                      ? sh_bin((zeta - sa.zeta_lo) * sa.zeta_scale, sa.zeta_bins - 1)
                                                      : sa.zeta_bins)], 1u);
                    if (sa.zeta_all)
                        sa.zeta_all[g] = zeta;
                }
            }

            // ---- O-O-O angles at i: the pairs (j, k), j < k, of the neighbours inside r_ang
            if (sa.ang_hist) { // wave-uniform
                const int m_ang = __popcll(wave_ballot(mine && r2 < sa.rang2)); // a prefix of the lanes
                for (int j = 0; j + 1 < m_ang; j++) {
                    const double jx = lane_f64(ex, j), jy = lane_f64(ey, j), jz = lane_f64(ez, j), j2 = lane_f64(r2, j);
                    if (lane > j && lane < m_ang) {
                        const double c = ((jx * ex + jy * ey) + jz * ez) / sqrt(j2 * r2);
                        const int kb = __builtin_isfinite(c) ? sh_bin((c + 1.0) * sa.ang_scale, sa.ang_bins - 1) : sa.ang_bins;
                        atomicAdd(&hw[sa.o_ang + kb], 1u); // lanes may share a bin
                    }
                }
            }

            if (sa.count && lane == 0)
                sa.count[g] = m;
            if (sa.nbr && lane < MMC_SHELL_NBR)
                sa.nbr[MMC_SHELL_NBR * g + lane] = jn; // -1 beyond the list
        }

        // the workgroup's counters added to the replica's (or the summed) ones and cleared, once every
        // wave has left the replica (the waves of a workgroup walk the same replicas: the barriers match)
        __syncthreads();
        const int64_t ro = sa.per_replica ? r : 0;
        for (int q = tid; q < hs; q += (int)blockDim.x) {
            const unsigned v = hw[q];
            if (v != 0u) {
                unsigned long long *dst;
                if (q == 0)
                    dst = sa.flagged + r;
                else if (q < sa.o_lsi)
                    dst = sa.rank_hist + ro * (sa.o_lsi - 1) + (q - 1);
                else if (q < sa.o_ang)
                    dst = sa.lsi_hist + ro * (sa.lsi_bins + 1) + (q - sa.o_lsi);
                else if (q < sa.o_zeta)
                    dst = sa.ang_hist + ro * (sa.ang_bins + 1) + (q - sa.o_ang);
                else
                    dst = sa.zeta_hist + ro * (sa.zeta_bins + 1) + (q - sa.o_zeta);
                atomicAdd(dst, (unsigned long long)v);
                hw[q] = 0u;
            }
        }
        if constexpr (!STAGE)
            __syncthreads(); // (STAGE: the barrier before the next replica's copy)
    }
}
