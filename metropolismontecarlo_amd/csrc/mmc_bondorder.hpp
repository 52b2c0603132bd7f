// mmc_bondorder.hpp -- bond-orientational order of 3-site molecules, read-only beside the chains:
//   k_bond_qlm       phase A, per molecule: its O-O neighbours inside r_nb sorted by distance, the
//                    harmonics of the nearest n_nb bonds and their mean q_lm, written with Q, the
//                    neighbours and a status word to a scratch record
//   k_bond_corr      phase B, per molecule: its own record and its neighbours' -- the bond
//                    correlations c_ij, the two windows, solid-like or not, the averaged qbar_l
//   k_bond_clusters  phase C, per replica: the clusters of solid-like molecules
// The arithmetic is stated in include/mmc_hip.h ("Bond order") and restated in numpy by
// tests/bond_order_ref.py.  The per-replica sums are k_local_qsum's (mmc_local.hpp).
//
// Phases A and B follow k_shell_order_wave (mmc_shell.hpp): a persistent workgroup takes a contiguous
// run of the chunk's molecules, its waves take the run's molecules of one replica after the other (A
// with the replica's O positions staged in LDS where they fit), and 32-bit counters in LDS, one set
// per workgroup, are added to the 64-bit global ones whenever the workgroup leaves a replica.
//
// Phase A, one molecule, one wave: scan_list and rank_sort (mmc_nbr.hpp), then
//   harmonics  lane k < n_i takes neighbour k: u = d / rho and, for m = 0 .. l, T_l^m(z) by the
//              header's recurrence and (x + i y)^m one complex product at a time -- scalars only, no
//              indexed registers -- written to the wave's [16][14] block in LDS
//   mean       lane t < 2 (l + 1) adds column t of that block in rank order (Re q_lm in lanes 0 .. l,
//              Im q_lm in lanes l + 1 .. 2 l + 1) and divides by n_i: the transposition through LDS
//              costs 2 (l + 1) writes and n_i reads per lane, against 2 lane reads per term of a
//              serial sum over the lanes
//   Q          lane m fetches its imaginary part from lane l + 1 + m; l + 1 lane reads, in rising m
// Phase B, one molecule, one wave: lane k < n_i loads neighbour k's record and adds its own 2 (l + 1)
// products (the molecule's own q_lm by lane reads: wave-uniform); ballots count the windows; lane
// t < 2 (l + 1) then adds component t of the neighbours' records in rank order for qbar_lm.
// Phase C, one workgroup per replica: labels (the molecule's index, or BO_NONE) in LDS; a round pushes
// the smaller label across every listed edge with atomicMin, towards whichever end is larger -- j in
// nb(i) does not imply i in nb(j), and pushing both ways is what symmetrises the graph -- until a round
// changes nothing.  The result is the lowest index of every component whatever the order.  Sizes by
// root in a second LDS array.
#pragma once
#include "mmc_shell.hpp"

#define BO_REC 16                 // doubles of a record: Re q_lm [l + 1], Im q_lm [l + 1], ..., [14] = Q
#define BO_Q 14
#define BO_COLS 14                // 2 (l + 1) at l = 6
#define BO_Y_BYTES (8 * MMC_BO_MAX_NB * BO_COLS) // a wave's block of harmonics
#define BO_UNDEF 0x100            // status: n_i in the low byte, and these
#define BO_FLAGGED 0x200
#define BO_NONE 0x7fffffff        // the label of a molecule that is not solid-like
#define BO_C_THREADS 256

struct BondArgs {
    const double *box_r;            // [R] per-replica boxes, or NULL: bv.box
    const double *norm;             // [7] N_m of the header
    // scratch of the chunk, indexed by (r - r0) N + i
    double *rec;                    // [.][BO_REC]
    int32_t *nb;                    // [.][MMC_BO_MAX_NB], -1 beyond n_i
    int32_t *st;                    // [.] status
    uint8_t *solid;                 // [.]
    // outputs on the device, indexed by the replica's index in the batch; each may be NULL
    unsigned long long *stats;      // [R][8], zeroed by the host
    unsigned long long *q_hist, *qbar_hist, *c_hist, *ab_hist, *size_hist; // zeroed by the host
    int32_t *nbr_out, *label_out;
    uint8_t *ab_out;
    double *q_all, *qbar_all;       // [.][N], indexed by (r - q_r0) N + i: the whole batch or the chunk
    double rnb2, K, a_lo, a_hi, b_lo, b_hi, q_scale, c_scale;
    int32_t l, n_nb, min_a, min_ab, q_bins, c_bins;
    int32_t per_replica, r0, nr, q_r0; // the chunk: replicas r0 .. r0 + nr - 1
};

// Q of the header from a wave that holds Re q_lm in lanes 0 .. l and Im q_lm in lanes l + 1 .. 2 l + 1
__device__ __forceinline__ double bo_norm2(double q, int lane, int l)
{
    const double im = wave_pick(q, min(lane + l + 1, 63));
    const double t = q * q + im * im; // lanes 0 .. l: t_m
    double Q = lane_f64(t, 0);
    for (int m = 1; m <= l; m++)
        Q = Q + 2.0 * lane_f64(t, m);
    return Q;
}

// REC, STAGE, grid: as k_shell_order_wave.
// dynamic LDS: [nw] lists of NBR_LIST_BYTES, [nw] blocks of BO_Y_BYTES, [hs] counters (defined,
// undefined, flagged, truncated, then q_hist's), then (STAGE) 3 N doubles at the next multiple of 16.
template <bool REC, bool STAGE>
__global__ __launch_bounds__(NBR_WAVES * 64) void k_bond_qlm(BatchView bv, const double *__restrict__ rec, BondArgs ba)
{
    extern __shared__ __align__(16) unsigned char bo_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nw = (int)(blockDim.x >> 6);
    const int n_mol = bv.n_mol, l = ba.l, cols = 2 * (l + 1);
    const int hs = 4 + (ba.q_hist ? ba.q_bins + 1 : 0);
    unsigned long long *const keys = reinterpret_cast<unsigned long long *>(bo_lds + (size_t)wv * NBR_LIST_BYTES);
    int *const idx = reinterpret_cast<int *>(keys + MMC_SHELL_CAP);
    double *const yb = reinterpret_cast<double *>(bo_lds + (size_t)nw * NBR_LIST_BYTES + (size_t)wv * BO_Y_BYTES);
    unsigned *const hw = reinterpret_cast<unsigned *>(bo_lds + (size_t)nw * (NBR_LIST_BYTES + BO_Y_BYTES));
    double *const pos = reinterpret_cast<double *>(
        bo_lds + (((size_t)nw * (NBR_LIST_BYTES + BO_Y_BYTES) + 4 * (size_t)hs + 15) & ~(size_t)15));
    for (int q = tid; q < hs; q += (int)blockDim.x)
        hw[q] = 0u;
    __syncthreads();

    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const Sites<REC, STAGE> sites{ bv, rec, pos };

    for (RunCursor rc(ba.nr, n_mol); rc.next();) { // the run's molecules of one replica of the chunk: [rc.lo, rc.hi)
        const int rl = rc.r, r = ba.r0 + rl;
        if constexpr (STAGE)
            stage_sites(sites, r);
        const BoxConsts bc = box_consts(ba.box_r ? ba.box_r[r] : bv.box);

        for (int i = rc.lo + wv; i < rc.hi; i += nw) {
            const int64_t g = (int64_t)rl * n_mol + i;      // in the chunk's scratch
            const int64_t go = (int64_t)r * n_mol + i;      // in the batch's outputs
            const int64_t gq = (int64_t)(r - ba.q_r0) * n_mol + i;
            double cx, cy, cz; // the wave's molecule: wave-uniform
            sites.get(r, i, cx, cy, cz);

            // ---- scan: the list, unsorted, in rising j
            int m;
            const bool over = !scan_list(sites, r, i, cx, cy, cz, bc, ba.rnb2, keys, idx, lane, m);

            if (over) { // wave-uniform
                if (lane == 0) {
                    atomicAdd(&hw[2], 1u);
                    if (ba.q_hist)
                        atomicAdd(&hw[4 + ba.q_bins], 1u);
                    ba.st[g] = BO_FLAGGED;
                    if (ba.q_all)
                        ba.q_all[gq] = nan;
                }
                if (lane < MMC_BO_MAX_NB) {
                    ba.nb[MMC_BO_MAX_NB * g + lane] = -1;
                    if (ba.nbr_out)
                        ba.nbr_out[MMC_BO_MAX_NB * go + lane] = -1;
                }
                continue;
            }

            // ---- sort: lane n's entry to slot rank(n); lane k then reads slot k
            unsigned long long key;
            int jn;
            rank_sort(keys, idx, m, lane, key, jn);

            // ---- harmonics: lane k < n is neighbour k of nb(i)
            const int n = min(m, ba.n_nb);
            const bool nbk = lane < n;
            if (!nbk)
                jn = -1;
            const double r2 = nbk ? __longlong_as_double((long long)key) : 1.0;
            const bool undef = n == 0 || wave_ballot(nbk && r2 == 0.0) != 0ULL; // wave-uniform
            if (nbk) {
                const double rho = sqrt(r2);
                double ox, oy, oz;
                sites.get(r, jn, ox, oy, oz);
                const double x = vector1D(cx, ox, bc) / rho, y = vector1D(cy, oy, bc) / rho, z = vector1D(cz, oz, bc) / rho;
                double c = 1.0, s = 0.0, tmm = 1.0; // (x + i y)^m and T_m^m
                for (int mm = 0; mm <= l; mm++) {
                    if (mm > 0) {
                        const double c1 = x * c - y * s, s1 = x * s + y * c;
                        c = c1;
                        s = s1;
                        tmm = tmm * (double)(2 * mm - 1);
                    }
                    double t = tmm; // T_n^m, n = m
                    if (mm < l) {
                        double t2 = tmm;
                        t = ((double)(2 * mm + 1) * z) * tmm; // n = m + 1
                        for (int nn = mm + 2; nn <= l; nn++) {
                            const double tn = ((((double)(2 * nn - 1) * z) * t) - ((double)(nn + mm - 1) * t2)) / (double)(nn - mm);
                            t2 = t;
                            t = tn;
                        }
                    }
                    const double A = ba.norm[mm] * t;
                    yb[lane * BO_COLS + mm] = A * c;
                    yb[lane * BO_COLS + l + 1 + mm] = A * s;
                }
            }
            wave_sync();

            // ---- mean: lane t < 2 (l + 1) owns one real or imaginary part
            double q = 0.0;
            if (lane < cols && n > 0) {
                q = yb[lane];
                for (int k = 1; k < n; k++)
                    q = q + yb[k * BO_COLS + lane];
                q = q / (double)n;
            }
            wave_sync(); // the block is rewritten by the wave's next molecule
            const double Q = bo_norm2(q, lane, l);
            const double ql = undef ? nan : sqrt(ba.K * Q);

            if (lane < BO_REC)
                ba.rec[BO_REC * g + lane] = lane < cols ? q : (lane == BO_Q ? Q : 0.0);
            if (lane < MMC_BO_MAX_NB) {
                ba.nb[MMC_BO_MAX_NB * g + lane] = jn;
                if (ba.nbr_out)
                    ba.nbr_out[MMC_BO_MAX_NB * go + lane] = jn;
            }
            if (lane == 0) {
                ba.st[g] = n | (undef ? BO_UNDEF : 0);
                atomicAdd(&hw[undef ? 1 : 0], 1u);
                if (m > ba.n_nb)
                    atomicAdd(&hw[3], 1u);
                if (ba.q_hist)
                    atomicAdd(&hw[4 + (undef ? ba.q_bins : sh_bin(ql * ba.q_scale, ba.q_bins - 1))], 1u);
                if (ba.q_all)
                    ba.q_all[gq] = ql;
            }
        }

        // the workgroup's counters added to the replica's (or the summed) ones and cleared
        __syncthreads();
        const int64_t ro = ba.per_replica ? r : 0;
        for (int q = tid; q < hs; q += (int)blockDim.x) {
            const unsigned v = hw[q];
            if (v != 0u) {
                if (q >= 4)
                    atomicAdd(ba.q_hist + ro * (ba.q_bins + 1) + (q - 4), (unsigned long long)v);
                else if (ba.stats)
                    atomicAdd(ba.stats + (int64_t)r * MMC_BO_STATS + q, (unsigned long long)v);
                hw[q] = 0u;
            }
        }
        if constexpr (!STAGE)
            __syncthreads(); // (STAGE: the barrier before the next replica's copy)
    }
}

// dynamic LDS: [hs] counters: qbar_hist's, c_hist's, ab_hist's, each only where asked for
__global__ __launch_bounds__(NBR_WAVES * 64) void k_bond_corr(BondArgs ba, int n_mol)
{
    extern __shared__ __align__(16) unsigned char bo_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nw = (int)(blockDim.x >> 6);
    const int l = ba.l, cols = 2 * (l + 1);
    const int o_c = ba.qbar_hist ? ba.q_bins + 1 : 0, o_ab = o_c + (ba.c_hist ? ba.c_bins + 1 : 0);
    const int hs = o_ab + (ba.ab_hist ? 289 : 0);
    unsigned *const hw = reinterpret_cast<unsigned *>(bo_lds);
    for (int q = tid; q < hs; q += (int)blockDim.x)
        hw[q] = 0u;
    __syncthreads();

    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (RunCursor rc(ba.nr, n_mol); rc.next();) {
        const int rl = rc.r, r = ba.r0 + rl;
        const int64_t gr = (int64_t)rl * n_mol; // the replica in the chunk's scratch

        for (int i = rc.lo + wv; i < rc.hi; i += nw) {
            const int64_t g = gr + i, go = (int64_t)r * n_mol + i;
            const int64_t gq = (int64_t)(r - ba.q_r0) * n_mol + i;
            const int sti = __builtin_amdgcn_readfirstlane(ba.st[g]);
            const int n = sti & 0xff;
            const bool def_i = (sti & (BO_UNDEF | BO_FLAGGED)) == 0;
            const double qi = lane < BO_REC ? ba.rec[BO_REC * g + lane] : 0.0; // lane t: component t; lane 14: Q_i
            const double Qi = lane_f64(qi, BO_Q);

            // ---- bonds: lane k < n is (i, j_k)
            const bool nbk = lane < n;
            const int jn = nbk ? ba.nb[MMC_BO_MAX_NB * g + lane] : 0;
            const int stj = nbk ? ba.st[gr + jn] : 0;
            const bool def_j = (stj & (BO_UNDEF | BO_FLAGGED)) == 0;
            const double *const rj = ba.rec + BO_REC * (gr + jn);
            double D = 0.0;
            for (int m = 0; m <= l; m++) {
                const double t = lane_f64(qi, m) * (nbk ? rj[m] : 0.0) + lane_f64(qi, l + 1 + m) * (nbk ? rj[l + 1 + m] : 0.0);
                D = m == 0 ? t : D + 2.0 * t;
            }
            const double Qj = nbk ? rj[BO_Q] : 0.0;
            const double c = D / (sqrt(Qi) * sqrt(Qj));
            const bool bond = nbk && def_i && def_j && Qi != 0.0 && Qj != 0.0 && __builtin_isfinite(c);
            if (ba.c_hist && nbk)
                atomicAdd(&hw[o_c + (bond ? sh_bin((c + 1.0) * ba.c_scale, ba.c_bins - 1) : ba.c_bins)], 1u);
            const int nA = __popcll(wave_ballot(bond && c >= ba.a_lo && c <= ba.a_hi));
            const int nB = __popcll(wave_ballot(bond && c >= ba.b_lo && c <= ba.b_hi));
            const bool solid = def_i && nA >= ba.min_a && nA + nB >= ba.min_ab;

            // ---- qbar_lm: lane t < 2 (l + 1) adds component t of the neighbours in rank order
            const bool def_bar = def_i && wave_ballot(nbk && !def_j) == 0ULL; // wave-uniform
            double qbar = nan;
            if (ba.qbar_hist || ba.qbar_all) { // wave-uniform
                double a = qi;
                for (int k = 0; k < n; k++) {
                    const int jk = __builtin_amdgcn_readlane(jn, k);
                    a = a + (lane < cols ? ba.rec[BO_REC * (gr + jk) + lane] : 0.0);
                }
                a = lane < cols ? a / (double)(n + 1) : 0.0;
                const double Qb = bo_norm2(a, lane, l);
                if (def_bar)
                    qbar = sqrt(ba.K * Qb);
            }

            if (lane == 0) {
                ba.solid[g] = solid ? 1 : 0;
                if (ba.ab_hist && def_i)
                    atomicAdd(&hw[o_ab + 17 * nA + nB], 1u);
                if (ba.qbar_hist)
                    atomicAdd(&hw[def_bar ? sh_bin(qbar * ba.q_scale, ba.q_bins - 1) : ba.q_bins], 1u);
                if (ba.qbar_all)
                    ba.qbar_all[gq] = qbar;
                if (ba.ab_out) {
                    ba.ab_out[2 * go] = (uint8_t)nA;
                    ba.ab_out[2 * go + 1] = (uint8_t)nB;
                }
            }
        }

        __syncthreads();
        const int64_t ro = ba.per_replica ? r : 0;
        for (int q = tid; q < hs; q += (int)blockDim.x) {
            const unsigned v = hw[q];
            if (v != 0u) {
                unsigned long long *dst;
                if (q < o_c)
                    dst = ba.qbar_hist + ro * (ba.q_bins + 1) + q;
                else if (q < o_ab)
                    dst = ba.c_hist + ro * (ba.c_bins + 1) + (q - o_c);
                else
                    dst = ba.ab_hist + ro * 289 + (q - o_ab);
                atomicAdd(dst, (unsigned long long)v);
                hw[q] = 0u;
            }
        }
        __syncthreads();
    }
}

// One workgroup per replica of the chunk.  dynamic LDS: labels [N], sizes [N], then 4 words (solid,
// clusters, largest, sum of s^2 -- at most N^2 < 2^32 for N <= MMC_BO_MAX_MOL).
__global__ __launch_bounds__(BO_C_THREADS) void k_bond_clusters(BondArgs ba, int n_mol)
{
    extern __shared__ __align__(16) unsigned char bo_lds[];
    int *const label = reinterpret_cast<int *>(bo_lds);
    unsigned *const size = reinterpret_cast<unsigned *>(bo_lds) + n_mol;
    unsigned *const tot = size + n_mol;
    const int tid = threadIdx.x, rl = blockIdx.x, r = ba.r0 + rl;
    const int64_t gr = (int64_t)rl * n_mol;

    for (int i = tid; i < n_mol; i += BO_C_THREADS) {
        label[i] = ba.solid[gr + i] ? i : BO_NONE;
        size[i] = 0u;
    }
    if (tid < 4)
        tot[tid] = 0u;
    __syncthreads();

    for (;;) { // labels only fall, and never below the lowest index of the component: it ends
        int changed = 0;
        for (int i = tid; i < n_mol; i += BO_C_THREADS) {
            if (!ba.solid[gr + i])
                continue;
            const int n = ba.st[gr + i] & 0xff;
            for (int k = 0; k < n; k++) {
                const int j = ba.nb[MMC_BO_MAX_NB * (gr + i) + k];
                if (!ba.solid[gr + j])
                    continue;
                const int li = label[i], lj = label[j]; // either may be stale: the next round sees it
                if (lj < li) {
                    atomicMin(&label[i], lj);
                    changed = 1;
                } else if (li < lj) {
                    atomicMin(&label[j], li);
                    changed = 1;
                }
            }
        }
        if (!__syncthreads_or(changed))
            break;
    }

    for (int i = tid; i < n_mol; i += BO_C_THREADS) {
        const int li = label[i];
        if (li != BO_NONE)
            atomicAdd(&size[li], 1u);
        if (ba.label_out)
            ba.label_out[(int64_t)r * n_mol + i] = li != BO_NONE ? li : -1;
    }
    __syncthreads();
    const int64_t ro = ba.per_replica ? r : 0;
    for (int i = tid; i < n_mol; i += BO_C_THREADS) {
        const unsigned s = size[i];
        if (s != 0u) { // i is the root of a cluster of s
            atomicAdd(&tot[0], s);
            atomicAdd(&tot[1], 1u);
            atomicMax(&tot[2], s);
            atomicAdd(&tot[3], s * s);
            if (ba.size_hist)
                atomicAdd(ba.size_hist + ro * (n_mol + 1) + s, 1ULL);
        }
    }
    __syncthreads();
    if (ba.stats && tid < 4)
        ba.stats[(int64_t)r * MMC_BO_STATS + 4 + tid] = tot[tid];
}
