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
//   scan     lane l takes j = l, l + 64, ...: r^2 of d(O_i, O_j) through vector1D_abs (the same bits as
//            the signed image squared), and keeps its four smallest in registers, sorted.  A lane
//            meets its j in rising order and a later key replaces an earlier one only when strictly
//            smaller, so inside a lane equal keys stay in index order.
//   bonds    lanes with r^2 < r_hb^2 append j to the wave's candidate list (ballot + prefix count);
//            the list is worked off 64 at a time: lane n takes candidate n's record and tests both
//            directions, i -> j through i's hydrogens and j -> i through j's, so no other
//            molecule's counters are touched.  r^2 of d(O_j, O_i) is bit for bit r^2 of d(O_i, O_j)
//            (vector1D of the negated difference is the negated image), so one gate serves both.
//   merge    four rounds: the 64-lane minimum of the lanes' smallest keys; lanes that tie (rare) are
//            told apart by a second minimum over j; the winner drops its head.
//   q        lanes 0..3 recompute the signed d of the four winners, lanes 0..5 take one pair (a, b)
//            each (one fp64 sqrt and one divide per lane), and the six terms are added in order.
// Counters: 32-bit, private to the wave in LDS (27 hydrogen-bond counters, q_bins of q), added to
// the 64-bit global ones whenever the wave leaves a replica -- integer adds, any order.
#pragma once
#include "mmc_tiles.hpp"

#define LO_WAVES 4              // waves per workgroup (fewer where the histograms would not fit: host)
#define LO_LDS_BYTES 65536      // dynamic LDS a workgroup may ask for without opting in
#define LO_CAND 128             // candidate slots per wave: at most 63 pending + 64 appended
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

__device__ __forceinline__ unsigned long long lo_shfl_xor(unsigned long long v, int m)
{
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, m, 64);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), m, 64);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long lo_wave_min(unsigned long long v)
{
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const unsigned long long o = lo_shfl_xor(v, m);
        v = o < v ? o : v;
    }
    return v; // in every lane
}
// one hydrogen of the donor: u = d(O_donor, H), v = d(O_donor, O_acceptor), vv = |v|^2
__device__ __forceinline__ bool lo_bond(double ux, double uy, double uz, double vx, double vy, double vz,
                                        double vv, double cos2)
{
    const double t = (ux * vx + uy * vy) + uz * vz;
    const double uu = (ux * ux + uy * uy) + uz * uz;
    return t > 0.0 && t * t >= cos2 * (uu * vv);
}

// REC: molecules are the 128-byte records of homogeneous batches; else the SoA arrays, slot a of
// molecule j at first0[j] + a.  STAGE: the replica's O positions are copied to LDS.
// grid: any number of workgroups of blockDim.x / 64 waves; workgroup g of G takes the molecules
// [R N g / G, R N (g + 1) / G) of the replica-major order.
// dynamic LDS: [nw][q_bins + 27] counters, [nw][LO_CAND] candidates, then (STAGE) 3 N doubles.
template <bool REC, bool STAGE>
__global__ __launch_bounds__(LO_WAVES * 64) void k_local_order_wave(BatchView bv, const double *__restrict__ rec,
                                                                    LocalArgs la)
{
    extern __shared__ __align__(16) unsigned char lo_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nw = (int)(blockDim.x >> 6);
    const int n_mol = bv.n_mol, nq = la.q_bins, hs = nq + LO_HB_ROWS;
    unsigned *const hw = reinterpret_cast<unsigned *>(lo_lds) + wv * hs;           // [27] then [q_bins]
    int *const cand = reinterpret_cast<int *>(lo_lds + 4 * (size_t)nw * hs) + wv * LO_CAND;
    // (4 nw (hs + LO_CAND) is a multiple of 8 only when nw hs is even: the host rounds it up)
    double *const pos = reinterpret_cast<double *>(lo_lds + ((4 * (size_t)nw * (hs + LO_CAND) + 15) & ~(size_t)15));
    for (int q = lane; q < hs; q += 64)
        hw[q] = 0u;
    wave_sync();

    const int64_t M = (int64_t)la.R * n_mol;
    const int64_t m0 = M * blockIdx.x / gridDim.x, m1 = M * (blockIdx.x + 1) / gridDim.x;

    // the O of molecule j (j < n_mol) of replica r
    auto oxygen = [&](int r, int j, double &x, double &y, double &z) {
        if constexpr (STAGE) {
            x = pos[j]; y = pos[n_mol + j]; z = pos[2 * n_mol + j];
        } else if constexpr (REC) {
            const double *p = rec + ((int64_t)r * n_mol + j) * MMC_RSTRIDE;
            const double2 v0 = *reinterpret_cast<const double2 *>(p);
            x = v0.x; y = v0.y; z = p[2];
        } else {
            const int64_t a0 = (int64_t)r * bv.atom_stride + bv.first0[j];
            x = bv.ax[a0]; y = bv.ay[a0]; z = bv.az[a0];
        }
    };

    for (int64_t s0 = m0; s0 < m1;) { // the run's molecules of one replica: [i_lo, i_hi) of replica r
        const int r = (int)(s0 / n_mol);
        const int i_lo = (int)(s0 - (int64_t)r * n_mol);
        const int i_hi = (int)min((int64_t)n_mol, (int64_t)i_lo + (m1 - s0));
        s0 += i_hi - i_lo;
        if constexpr (STAGE) {
            __syncthreads(); // every wave has left the previous replica's positions
            for (int j = tid; j < n_mol; j += (int)blockDim.x) {
                double x, y, z;
                if constexpr (REC) {
                    const double *p = rec + ((int64_t)r * n_mol + j) * MMC_RSTRIDE;
                    const double2 v0 = *reinterpret_cast<const double2 *>(p);
                    x = v0.x; y = v0.y; z = p[2];
                } else {
                    const int64_t a0 = (int64_t)r * bv.atom_stride + bv.first0[j];
                    x = bv.ax[a0]; y = bv.ay[a0]; z = bv.az[a0];
                }
                pos[j] = x; pos[n_mol + j] = y; pos[2 * n_mol + j] = z;
            }
            __syncthreads();
        }
        const BoxConsts bc = box_consts(la.box_r ? la.box_r[r] : bv.box);

        for (int i = i_lo + wv; i < i_hi; i += nw) {
            double ci[9]; // the wave's molecule: wave-uniform
            load_sites9<REC>(bv, rec, r, i, ci); // O, H, H
            double ui[2][3]; // d(O_i, H_i,h)
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int d = 0; d < 3; d++)
                    ui[h][d] = vector1D(ci[d], ci[3 + 3 * h + d], bc);

            unsigned long long k0 = ~0ULL, k1 = ~0ULL, k2 = ~0ULL, k3 = ~0ULL;
            int j0 = 0x7fffffff, j1 = 0x7fffffff, j2 = 0x7fffffff, j3 = 0x7fffffff;
            int n_cand = 0, don = 0, acc = 0;

            // candidates [0, n) of the list, one per lane (n <= 64): both directions of each pair
            auto bonds = [&](int n) {
                bool b1 = false, b2 = false, b3 = false, b4 = false;
                if (lane < n) {
                    const int j = cand[lane];
                    double cj[9];
                    load_sites9<REC>(bv, rec, r, j, cj);
                    const double vx = vector1D(ci[0], cj[0], bc), vy = vector1D(ci[1], cj[1], bc),
                                 vz = vector1D(ci[2], cj[2], bc);
                    const double vv = (vx * vx + vy * vy) + vz * vz;
                    b1 = lo_bond(ui[0][0], ui[0][1], ui[0][2], vx, vy, vz, vv, la.cos2);
                    b2 = lo_bond(ui[1][0], ui[1][1], ui[1][2], vx, vy, vz, vv, la.cos2);
                    const double wx = vector1D(cj[0], ci[0], bc), wy = vector1D(cj[1], ci[1], bc),
                                 wz = vector1D(cj[2], ci[2], bc);
                    const double ww = (wx * wx + wy * wy) + wz * wz;
                    b3 = lo_bond(vector1D(cj[0], cj[3], bc), vector1D(cj[1], cj[4], bc), vector1D(cj[2], cj[5], bc),
                                 wx, wy, wz, ww, la.cos2);
                    b4 = lo_bond(vector1D(cj[0], cj[6], bc), vector1D(cj[1], cj[7], bc), vector1D(cj[2], cj[8], bc),
                                 wx, wy, wz, ww, la.cos2);
                }
                don += __popcll(wave_ballot(b1)) + __popcll(wave_ballot(b2));
                acc += __popcll(wave_ballot(b3)) + __popcll(wave_ballot(b4));
            };

            for (int jb = 0; jb < n_mol; jb += 64) {
                const int j = jb + lane;
                const bool valid = j < n_mol && j != i;
                double x, y, z;
                oxygen(r, min(j, n_mol - 1), x, y, z);
                const double dx = vector1D_abs(ci[0], x, bc), dy = vector1D_abs(ci[1], y, bc),
                             dz = vector1D_abs(ci[2], z, bc);
                const double r2 = (dx * dx + dy * dy) + dz * dz;
                const unsigned long long k = valid ? (unsigned long long)__double_as_longlong(r2) : ~0ULL;
                // sorted insertion behind equal keys
                const bool c0 = k < k0, c1 = k < k1, c2 = k < k2, c3 = k < k3;
                k3 = c2 ? k2 : (c3 ? k : k3); j3 = c2 ? j2 : (c3 ? j : j3);
                k2 = c1 ? k1 : (c2 ? k : k2); j2 = c1 ? j1 : (c2 ? j : j2);
                k1 = c0 ? k0 : (c1 ? k : k1); j1 = c0 ? j0 : (c1 ? j : j1);
                k0 = c0 ? k : k0;             j0 = c0 ? j : j0;

                const bool near = valid && r2 < la.rhb2;
                const unsigned long long nm = wave_ballot(near);
                if (nm != 0ULL) { // wave-uniform
                    if (near)
                        cand[n_cand + lanes_below(nm)] = j; // n_cand <= 63 here: the slot is < LO_CAND
                    n_cand += __popcll(nm);
                    wave_sync();
                    if (n_cand >= 64) {
                        bonds(64);
                        const int rest = n_cand - 64; // <= 63: one lane each
                        const int mv = lane < rest ? cand[64 + lane] : 0;
                        wave_sync();
                        if (lane < rest)
                            cand[lane] = mv;
                        wave_sync();
                        n_cand = rest;
                    }
                }
            }
            if (n_cand > 0)
                bonds(n_cand);
            wave_sync(); // the list is rewritten by the wave's next molecule

            // the four nearest of the wave: (key, j) minimum of the lanes' heads, four times
            unsigned long long wk[4];
            int wj[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const unsigned long long m = lo_wave_min(k0);
                const unsigned long long tie = wave_ballot(k0 == m);
                int jw;
                if (__popcll(tie) > 1) { // wave-uniform: equal r^2 bits in several lanes: the lowest j
                    const unsigned long long jm =
                        lo_wave_min(k0 == m ? (unsigned long long)(unsigned)j0 : ~0ULL);
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
            oxygen(r, min(max(ja, 0), n_mol - 1), ox, oy, oz); // (n_mol >= 5: ja is a molecule; clamped all the same)
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
__global__ __launch_bounds__(LO_WAVES * 64) void k_local_qsum(const double *__restrict__ q_all, double *out,
                                                              int n_mol, int R)
{
    const int lane = threadIdx.x & 63;
    const int r = (int)blockIdx.x * LO_WAVES + (int)(threadIdx.x >> 6);
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
