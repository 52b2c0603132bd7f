// mmc_sofq.hpp -- partial structure factors of every replica, read-only beside the chains:
//   k_sofq_wave     rho_a(n) = sum_i e^{i 2 pi n . r_{i,a} / L} for the three atom slots over the half
//                   space of integer vectors 0 < |n|^2 <= n_max^2, and per shell s = |n|^2 the six sums
//                   of 2 Q(rho_a.re rho_b.re + rho_a.im rho_b.im) as 64-bit integers
//   k_sofq_reduce   sq_sum = the per-replica integers times 2^-24, added in fp64 in replica order
//
// The shape is k_recip_long_lds' (mmc_total.hpp): a workgroup builds the six phase factors of every
// atom of a replica in LDS (48 bytes per atom, slot-major: 147 KB at 1024 molecules) and its waves
// take (nx, ny) columns from a queue.  Lane = molecule: lane l adds molecules l, l + 64, ... in that
// order, the 64 lane sums go through wave_sum, and one wave computes a given rho_a(n) alone -- the
// bits of every rho do not depend on the launch.  The arithmetic is the reference's recurrence
// (Ewald/ewalds.jl:538-604, powers :575-585): x1^nx and y1^|ny| by repeated c_mul from 1, the
// conjugate for ny < 0, xy = c_mul(ex, ey), p_k = c_mul(p_{k-1}, z1) from p_0 = 1, the term
// c_mul(xy, p_k) for nz = k and c_mul(xy, conj(p_k)) for nz = -k.
//
// A column holds nz = -kz .. kz with kz up to 32: 4 (2 kz + 1) accumulators per slot are too many for
// one pass, so the |nz| are walked in blocks of SQ_B (k0 = 0, SQ_B, ...), one slot at a time: 4 SQ_B
// accumulators.  The block's first power z1^k0 is made by the same k0 products from 1 that a single
// pass would have made -- the sequence of products is part of the definition, and restarting it with
// another one would change bits.  What that costs: x1^nx, y1^|ny| and z1^k0 again per (column, block,
// slot, molecule), about as many products as the block's own at n_max = 32.
//
// After the wave sums the block's 2 SQ_B vectors sit one per lane (lane j: nz = k0 + j, lane SQ_B + j:
// nz = -(k0 + j)) for each slot, so the six products, Q and the six 64-bit atomics to the replica's
// counters in global scratch are one vector instruction each per block, not per vector.
// Q(v) = v 2^24 rounded to nearest even by the 1.5 2^52 add of mmc_orient.hpp.
//
// Units: (replica, part) with `split` parts per replica; part p of a replica takes the columns
// p, p + split, ... of the work-ordered list.  Many replicas: split = 1 and a persistent workgroup
// takes units g, g + G, ...  Few replicas: split > 1 workgroups share a replica's columns, each
// rebuilding the phases.  All sums are integers: the result does not depend on either.
#pragma once
#include "mmc_orient.hpp"

#define SQ_WAVES 8 // waves per workgroup: 256 registers per lane, room for 4 SQ_B accumulators
#define SQ_B 16    // |nz| per block
static_assert(2 * SQ_B <= 64, "a block's vectors sit one per lane");
static_assert(48 * 3 * MMC_SOFQ_MAX_MOL + 64 <= 160 * 1024, "the phases of MMC_SOFQ_MAX_MOL molecules fit 160 KB of LDS");

struct SofqArgs {
    const double *box_r;     // [R] per-replica boxes, or NULL: bv.box
    const int32_t *cols;     // [n_cols] nx | (ny + 64) << 8 | kz_max << 16, most work first
    unsigned long long *cnt; // [n_rep][6][S] zeroed by the host
    int32_t n_cols, S;       // S = n_max^2 + 1
    int32_t r0, n_rep;       // replicas r0 .. r0 + n_rep - 1
    int32_t split;           // parts per replica
};

__device__ __forceinline__ double sq_first_lane(double v)
{
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)b);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// Q(v) = v 2^24 rounded to nearest, ties to even, as a 64-bit integer (mod 2^64): or_quant's add
__device__ __forceinline__ unsigned long long sq_quant(double v)
{
    return (unsigned long long)__double_as_longlong(v * MMC_SOFQ_SCALE + OR_MAGIC) - OR_MAGIC_BITS;
}

// x^n, n >= 0, by n products from 1 (the first, 1 x, is exact)
__device__ __forceinline__ cplx sq_pow(cplx x, int n)
{
    cplx p = { 1.0, 0.0 };
    for (int k = 0; k < n; k++)
        p = c_mul(p, x);
    return p;
}

// rho of one slot for the block k0 .. k0 + kc - 1 of column (nx, ny): lane j < kc gets nz = k0 + j,
// lane SQ_B + j gets nz = -(k0 + j); the other lanes 0.
__device__ __forceinline__ void sq_block(const double *ph /* [n_mol][6] of the slot */, int n_mol, int nx, int ny,
                                         int k0, int kc, int lane, double &res_re, double &res_im)
{
    const int aky = ny < 0 ? -ny : ny;
    double acc[4 * SQ_B];
#pragma unroll
    for (int q = 0; q < 4 * SQ_B; q++)
        acc[q] = 0.0;
    for (int m = lane; m < n_mol; m += 64) {
        const double2 px = *reinterpret_cast<const double2 *>(ph + 6 * m),
                      py = *reinterpret_cast<const double2 *>(ph + 6 * m + 2),
                      pz = *reinterpret_cast<const double2 *>(ph + 6 * m + 4);
        const cplx x1 = { px.x, px.y }, y1 = { py.x, py.y }, z1 = { pz.x, pz.y };
        const cplx ex = sq_pow(x1, nx);
        cplx ey = sq_pow(y1, aky);
        if (ny < 0)
            ey = c_conj(ey);
        const cplx xy = c_mul(ex, ey);
        cplx p = sq_pow(z1, k0);
#pragma unroll
        for (int j = 0; j < SQ_B; j++) {
            if (j < kc) { // (wave-uniform)
                if (j > 0)
                    p = c_mul(p, z1);
                const cplx tp = c_mul(xy, p), tm = c_mul(xy, c_conj(p));
                acc[4 * j] += tp.re;
                acc[4 * j + 1] += tp.im;
                acc[4 * j + 2] += tm.re;
                acc[4 * j + 3] += tm.im;
            }
        }
    }
    res_re = 0.0;
    res_im = 0.0;
#pragma unroll
    for (int j = 0; j < SQ_B; j++) {
        if (j < kc) {
            const double pr = sq_first_lane(wave_sum(acc[4 * j])), pi = sq_first_lane(wave_sum(acc[4 * j + 1]));
            const double mr = sq_first_lane(wave_sum(acc[4 * j + 2])), mi = sq_first_lane(wave_sum(acc[4 * j + 3]));
            res_re = lane == j ? pr : (lane == SQ_B + j ? mr : res_re);
            res_im = lane == j ? pi : (lane == SQ_B + j ? mi : res_im);
        }
    }
}

// REC: molecules are the 128-byte records of homogeneous batches; else the SoA arrays (a batch holds
// three-atom molecules only).
// grid: any number of workgroups of SQ_WAVES waves; dynamic LDS 144 n_mol bytes.
template <bool REC>
__global__ __launch_bounds__(SQ_WAVES * 64) void k_sofq_wave(BatchView bv, const double *__restrict__ rec, SofqArgs sa)
{
    extern __shared__ __align__(16) double sq_lds[]; // [3][n_mol][6] cos x, sin x, cos y, sin y, cos z, sin z
    __shared__ int next_col;
    const int n_mol = bv.n_mol, tid = threadIdx.x, lane0 = tid & 63;
    const int S = sa.S, split = sa.split;
    const int n_units = sa.n_rep * split;
    for (int u = blockIdx.x; u < n_units; u += (int)gridDim.x) {
        const int rl = u / split, part = u - rl * split, r = sa.r0 + rl;
        const double L = sa.box_r ? sa.box_r[r] : bv.box;
        __syncthreads(); // (the previous unit's columns are done with the phases and the queue)
        if (tid == 0)
            next_col = 0;
        for (int m = tid; m < n_mol; m += SQ_WAVES * 64) {
            double t[9];
            if constexpr (REC) {
                const double2 *src = reinterpret_cast<const double2 *>(rec + ((int64_t)r * n_mol + m) * MMC_RSTRIDE);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const double2 v = src[q];
                    t[2 * q] = v.x;
                    t[2 * q + 1] = v.y;
                }
                t[8] = src[4].x;
            } else {
                const int64_t a0 = (int64_t)r * bv.atom_stride + bv.first0[m];
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    t[3 * a] = bv.ax[a0 + a]; t[3 * a + 1] = bv.ay[a0 + a]; t[3 * a + 2] = bv.az[a0 + a];
                }
            }
#pragma unroll
            for (int a = 0; a < 3; a++) {
                double *o = sq_lds + ((int64_t)a * n_mol + m) * 6;
                double sn, cs;
                sincos_moderate(MMC_TWOPI * t[3 * a] / L, sn, cs); o[0] = cs; o[1] = sn;
                sincos_moderate(MMC_TWOPI * t[3 * a + 1] / L, sn, cs); o[2] = cs; o[3] = sn;
                sincos_moderate(MMC_TWOPI * t[3 * a + 2] / L, sn, cs); o[4] = cs; o[5] = sn;
            }
        }
        __syncthreads();
        unsigned long long *const cnt = sa.cnt + (int64_t)rl * 6 * S;
        for (;;) {
            int lane = lane0;
            asm volatile("" : "+v"(lane)); // keep lane-derived values of the inlined blocks out of LICM
            int slot = 0;
            if (lane == 0)
                slot = atomicAdd(&next_col, 1);
            slot = __builtin_amdgcn_readfirstlane(slot);
            const int ci = part + slot * split;
            if (ci >= sa.n_cols)
                break;
            const int c = sa.cols[ci];
            const int nx = c & 0xff, ny = ((c >> 8) & 0xff) - 64, kzm = c >> 16;
            for (int k0 = 0; k0 <= kzm; k0 += SQ_B) {
                const int kc = min(SQ_B, kzm - k0 + 1);
                double re[3], im[3];
#pragma unroll
                for (int a = 0; a < 3; a++)
                    sq_block(sq_lds + (int64_t)a * n_mol * 6, n_mol, nx, ny, k0, kc, lane, re[a], im[a]);
                // lane j: the vector (nx, ny, nz); the half space keeps nz > 0 only of column (0, 0)
                const bool minus = lane >= SQ_B;
                const int j = minus ? lane - SQ_B : lane, k = k0 + j;
                const int s = nx * nx + ny * ny + k * k;
                const bool ok = lane < 2 * SQ_B && j < kc && !(minus && k == 0) && !(nx == 0 && ny == 0 && (minus || k == 0))
                                && s < S;
                if (ok) {
                    int row = 0;
#pragma unroll
                    for (int a = 0; a < 3; a++)
#pragma unroll
                        for (int b = a; b < 3; b++) {
                            const double v = re[a] * re[b] + im[a] * im[b];
                            const unsigned long long q = sq_quant(v);
                            atomicAdd(&cnt[(int64_t)row * S + s], 2ull * q);
                            row++;
                        }
                }
            }
        }
    }
}

// sum[e] (+)= sum over the chunk's replicas, ascending, of (double)cnt[r][e] 2^-24
__global__ void k_sofq_reduce(const unsigned long long *__restrict__ cnt, double *sum, int n_rep, int n_ent, int first)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_ent)
        return;
    double acc = first ? 0.0 : sum[e];
#pragma unroll 8
    for (int r = 0; r < n_rep; r++)
        acc += (double)(long long)cnt[(int64_t)r * n_ent + e] * (1.0 / MMC_SOFQ_SCALE);
    sum[e] = acc;
}
