// mmc_local.hpp -- first-shell structure of 3-site molecules, read-only beside the chains:
//   k_local_order_wave   per molecule: its four nearest O-O neighbours, the tetrahedral order
//                        parameter q of them, and its donated / accepted hydrogen bonds
//   k_local_qsum         the sum of a replica's finite q_i in a fixed order
// The arithmetic is stated in include/mmc_hip.h ("Local order") and restated in numpy by
// tests/local_order_ref.py; slot 0 of a molecule is the heavy atom, slots 1 and 2 the hydrogens.
//
// The scheme is the wave-per-unit one of mmc_struct.hpp with the molecule as the unit.  A persistent
// workgroup takes a contiguous run of the R N molecules; for every replica its run touches it copies
// the replica's O positions into LDS once (24 bytes per molecule, SoA so that consecutive lanes read
// consecutive doubles), and its waves then take the run's molecules of that replica in turn.  The
// only workgroup barriers are the two around that copy; inside a molecule a wave waits for nobody.
// Where the positions do not fit beside the histograms (STAGE = false) the lanes read them from
// the 128-byte records or the SoA arrays instead.
//
// One molecule i, one wave:
//   scan     scan_candidates (mmc_nbr.hpp): lane l takes j = l, l + 64, ... and, through `nearest`,
//            keeps its four smallest r^2 of d(O_i, O_j) in registers, sorted.  A lane
//            meets its j in rising order and a later key replaces an earlier one only when strictly
//            smaller, so inside a lane equal keys stay in index order.
//   bonds    the candidates inside r_hb come 64 at a time: lane n takes candidate n's record and
//            tests both directions (HbPair), i -> j through i's hydrogens and j -> i through j's,
//            so no other molecule's counters are touched.
//   merge    four rounds: the 64-lane minimum of the lanes' smallest keys; lanes that tie (rare) are
//            told apart by a second minimum over j; the winner drops its head.
//   q        lanes 0..3 recompute the signed d of the four winners, lanes 0..5 take one pair (a, b)
//            each (one fp64 sqrt and one divide per lane), and the six terms are added in order.
// Counters: 32-bit, private to the wave in LDS (27 hydrogen-bond counters, q_bins of q), added to
// the 64-bit global ones whenever the wave leaves a replica -- integer adds, any order.
#pragma once
#include "mmc_nbr.hpp"

#define MMC_LOCAL_MAX_BINS 4096
#define LO_HB_ROWS 27           // [3][9]: donated, accepted, total over n = 0..8

struct LocalArgs {
    const double *box_r;        // [R] per-replica boxes, or NULL: bv.box
    unsigned long long *hb_hist; // [27] or [R][27], zeroed by the host
    unsigned long long *q_hist;  // [q_bins] or [R][q_bins], zeroed by the host
    double *q_all;              // [R][N] or NULL
    int32_t *nbr;               // [R][N][4] or NULL
    uint8_t *hb;                // [R][N][2] or NULL
    double rhb2, cos2, q_scale; // r_hb r_hb, cos_hb cos_hb, q_bins / 4.0
    int32_t q_bins, per_replica;
    int32_t R;
};

// REC: molecules are the 128-byte records of homogeneous batches; else the SoA arrays, slot a of
// molecule j at first0[j] + a.  STAGE: the replica's O positions are copied to LDS.
// grid: any number of workgroups of blockDim.x / 64 waves; workgroup g of G takes the molecules
// [R N g / G, R N (g + 1) / G) of the replica-major order.
// dynamic LDS: [nw][q_bins + 27] counters, [nw][NBR_CAND] candidates, then (STAGE) 3 N doubles.
template <bool REC, bool STAGE>
__global__ __launch_bounds__(NBR_WAVES * 64) void k_local_order_wave(BatchView bv, const double *__restrict__ rec,
                                                                    LocalArgs la)
{
    extern __shared__ __align__(16) unsigned char lo_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nw = (int)(blockDim.x >> 6);
    const int n_mol = bv.n_mol, nq = la.q_bins, hs = nq + LO_HB_ROWS;
    unsigned *const hw = reinterpret_cast<unsigned *>(lo_lds) + wv * hs;           // [27] then [q_bins]
    int *const cand = reinterpret_cast<int *>(lo_lds + 4 * (size_t)nw * hs) + wv * NBR_CAND;
    // (4 nw (hs + NBR_CAND) is a multiple of 8 only when nw hs is even: the host rounds it up)
    double *const pos = reinterpret_cast<double *>(lo_lds + ((4 * (size_t)nw * (hs + NBR_CAND) + 15) & ~(size_t)15));
    for (int q = lane; q < hs; q += 64)
        hw[q] = 0u;
    wave_sync();

    const Sites<REC, STAGE> sites{ bv, rec, pos };

    for (RunCursor rc(la.R, n_mol); rc.next();) { // the run's molecules of one replica: [rc.lo, rc.hi) of replica r
        const int r = rc.r;
        if constexpr (STAGE)
            stage_sites(sites, r);
        const BoxConsts bc = box_consts(la.box_r ? la.box_r[r] : bv.box);

        for (int i = rc.lo + wv; i < rc.hi; i += nw) {
            double ci[9]; // the wave's molecule: wave-uniform
            load_sites9<REC>(bv, rec, r, i, ci); // O, H, H
            double ui[2][3]; // d(O_i, H_i,h)
            hb_arms(ci, bc, ui);

            unsigned long long k0 = ~0ULL, k1 = ~0ULL, k2 = ~0ULL, k3 = ~0ULL;
            int j0 = 0x7fffffff, j1 = 0x7fffffff, j2 = 0x7fffffff, j3 = 0x7fffffff;
            int don = 0, acc = 0;

            // the lane's four smallest keys, sorted: insertion behind equal keys
            auto nearest = [&](int j, bool valid, double r2) {
                const unsigned long long k = valid ? (unsigned long long)__double_as_longlong(r2) : ~0ULL;
                const bool c0 = k < k0, c1 = k < k1, c2 = k < k2, c3 = k < k3;
                k3 = c2 ? k2 : (c3 ? k : k3); j3 = c2 ? j2 : (c3 ? j : j3);
                k2 = c1 ? k1 : (c2 ? k : k2); j2 = c1 ? j1 : (c2 ? j : j2);
                k1 = c0 ? k0 : (c1 ? k : k1); j1 = c0 ? j0 : (c1 ? j : j1);
                k0 = c0 ? k : k0;             j0 = c0 ? j : j0;
            };
            // candidates [0, n) of the list, one per lane (n <= 64): both directions of each pair
            auto bonds = [&](int n) {
                bool b1 = false, b2 = false, b3 = false, b4 = false;
                if (lane < n) {
                    const int j = cand[lane];
                    double cj[9];
                    load_sites9<REC>(bv, rec, r, j, cj);
                    const HbPair hp(ci, ui, cj, bc);
                    b1 = hp.bonded(0, la.cos2);
                    b2 = hp.bonded(1, la.cos2);
                    b3 = hp.bonded(2, la.cos2);
                    b4 = hp.bonded(3, la.cos2);
                }
                don += __popcll(wave_ballot(b1)) + __popcll(wave_ballot(b2));
                acc += __popcll(wave_ballot(b3)) + __popcll(wave_ballot(b4));
            };
            scan_candidates(sites, r, i, ci[0], ci[1], ci[2], bc, la.rhb2, cand, lane, nearest, bonds);

            // the four nearest of the wave: (key, j) minimum of the lanes' heads, four times
            unsigned long long wk[4];
            int wj[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const unsigned long long m = wave_min_u64(k0);
                const unsigned long long tie = wave_ballot(k0 == m);
                int jw;
                if (__popcll(tie) > 1) { // wave-uniform: equal r^2 bits in several lanes: the lowest j
                    const unsigned long long jm =
                        wave_min_u64(k0 == m ? (unsigned long long)(unsigned)j0 : ~0ULL);
                    jw = (int)(unsigned)jm;
                } else {
                    jw = __builtin_amdgcn_readlane(j0, __builtin_ctzll(tie));
                }
                wk[q] = m;
                wj[q] = jw;
                if (k0 == m && j0 == jw) { // the winner drops its head
                    k0 = k1; k1 = k2; k2 = k3; k3 = ~0ULL;
                    j0 = j1; j1 = j2; j2 = j3; j3 = 0x7fffffff;
                }
            }

            // q: lanes 0..3 hold d of rank lane, lanes 0..5 one pair each
            const int ra = lane & 3;
            const int ja = ra == 0 ? wj[0] : ra == 1 ? wj[1] : ra == 2 ? wj[2] : wj[3];
            double ox, oy, oz;
            sites.get(r, min(max(ja, 0), n_mol - 1), ox, oy, oz); // (n_mol >= 5: ja is a molecule; clamped all the same)
            const double ex = vector1D(ci[0], ox, bc), ey = vector1D(ci[1], oy, bc), ez = vector1D(ci[2], oz, bc);
            const double e2 = (ex * ex + ey * ey) + ez * ez;
            const int pa = lane < 3 ? 0 : (lane < 5 ? 1 : 2);                       // (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
            const int pb = lane < 3 ? lane + 1 : (lane < 5 ? lane - 1 : 3);
            const int la_ = lane < 6 ? pa : 0, lb_ = lane < 6 ? pb : 1;
            const double ax = wave_pick(ex, la_), ay = wave_pick(ey, la_), az = wave_pick(ez, la_), a2 = wave_pick(e2, la_);
            const double bx = wave_pick(ex, lb_), by = wave_pick(ey, lb_), bz = wave_pick(ez, lb_), b2 = wave_pick(e2, lb_);
            const double cab = ((ax * bx + ay * by) + az * bz) / sqrt(a2 * b2);
            const double term = (cab + 1.0 / 3.0) * (cab + 1.0 / 3.0);
            double ssum = wave_pick(term, 0);
#pragma unroll
            for (int p = 1; p < 6; p++)
                ssum = ssum + wave_pick(term, p);
            double qi = 1.0 - 0.375 * ssum;
            if (wk[0] == 0ULL || wk[1] == 0ULL || wk[2] == 0ULL || wk[3] == 0ULL) // a coincident neighbour
                qi = __longlong_as_double(0x7ff8000000000000LL);

            const int dn = min(don, 8), an = min(acc, 8), tn = min(don + acc, 8);
            if (lane == 0) {
                const int64_t g = (int64_t)r * n_mol + i;
                hw[dn] += 1u;
                hw[9 + an] += 1u;
                hw[18 + tn] += 1u;
                if (__builtin_isfinite(qi)) {
                    const double fk = floor((qi + 3.0) * la.q_scale);
                    const int kb = (int)fmin(fmax(fk, 0.0), (double)(nq - 1));
                    hw[LO_HB_ROWS + kb] += 1u;
                }
                if (la.q_all)
                    la.q_all[g] = qi;
                if (la.nbr)
                    *reinterpret_cast<int4 *>(la.nbr + 4 * g) = make_int4(wj[0], wj[1], wj[2], wj[3]);
                if (la.hb) {
                    la.hb[2 * g] = (uint8_t)dn;
                    la.hb[2 * g + 1] = (uint8_t)an;
                }
            }
        }

        // this wave's counters added to the replica's (or the summed) ones and cleared
        wave_sync();
        const int64_t ro = la.per_replica ? r : 0;
        for (int q = lane; q < hs; q += 64) {
            const unsigned v = hw[q];
            if (v != 0u) {
                unsigned long long *dst = q < LO_HB_ROWS ? la.hb_hist + ro * LO_HB_ROWS + q
                                                         : la.q_hist + ro * nq + (q - LO_HB_ROWS);
                atomicAdd(dst, (unsigned long long)v);
                hw[q] = 0u;
            }
        }
        wave_sync();
    }
}

// One wave per replica: lane l adds the finite q_i of molecules i = l, l + 64, ... in that order, then
// the 64 lane sums are added by wave_sum_rows (DPP, fixed order): the bits do not depend on the
// launch.  out[r] = (sum, number of finite q_i).
__global__ __launch_bounds__(NBR_WAVES * 64) void k_local_qsum(const double *__restrict__ q_all, double *out,
                                                              int n_mol, int R)
{
    const int lane = threadIdx.x & 63;
    const int r = (int)blockIdx.x * NBR_WAVES + (int)(threadIdx.x >> 6);
    if (r >= R)
        return;
    double acc = 0.0;
    int cnt = 0;
    for (int i = lane; i < n_mol; i += 64) {
        const double q = q_all[(int64_t)r * n_mol + i];
        if (__builtin_isfinite(q)) {
            acc += q;
            cnt++;
        }
    }
    const double s = wave_sum_rows(acc);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        cnt += __shfl_xor(cnt, off, 64);
    if (lane == 0) {
        out[2 * (int64_t)r] = s;
        out[2 * (int64_t)r + 1] = (double)cnt;
    }
}
