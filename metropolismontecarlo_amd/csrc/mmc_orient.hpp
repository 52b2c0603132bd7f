// mmc_orient.hpp -- orientational pair correlations of every replica, read-only beside the chains:
//   k_orient_corr_wave   pair count, sum u_i.u_j, sum 3 (u_i.rhat)(u_j.rhat) - u_i.u_j and sum P2(u_i.u_j)
//                        per bin of the slot-0 separation, every pair i < j once
//
// The separation and its bin are row (0,0) of k_rdf_sites_wave bit for bit (mmc_struct.hpp: st_image,
// r^2 = (xx xx + yy yy) + zz zz; mmc_tiles.hpp: tile_bin).  The axis u_i is the unit vector of
// k_dipoles' mu_i = (q_0 d_0 + q_1 d_1) + q_2 d_2, d_a = vector1D(COM, atom a); u = mu / sqrt(n^2),
// n^2 = (mu_x^2 + mu_y^2) + mu_z^2, and u = 0 when n^2 is 0 or not finite.  Per pair
//     c  = (u_i.x u_j.x + u_i.y u_j.y) + u_i.z u_j.z
//     p2 = 1.5 c^2 - 0.5
//     hd = 3 (u_i.d)(u_j.d) / r^2 - c          (0 when r^2 = 0)
// and rows 1, 2, 3 add Q(c), Q(hd), Q(p2), Q(v) = round-to-nearest-even of v 2^30 as a 64-bit
// integer: all four rows are integer sums, so no order of lanes, waves, flushes or atomics can change
// a bit of the result.
//
// The tiles of the i < j triangle and a wave's run of them are mmc_tiles.hpp's.  Lane n keeps
// neighbour n of block k across a row of tiles -- here six doubles, site 0 and u, not nine.  u costs
// a square root and three divisions: it is computed once per (replica, block) by the lane that loads
// the record.  The chosen side: at the start of a tile the 64 lanes load block c's records and
// compute their u as well, and the walk over the chosen
// molecules pulls the six values out with v_readlane (twelve per chosen molecule, against ~70 vector
// instructions per pair row), so every vector instruction of the pair has them as scalar operands
// and the hot loop has no memory load at all.  (The alternative, a [R][N][8] array of site 0 and u
// in the observables' scratch read through scalar loads, costs 64 bytes per molecule -- 2.9 GB at
// 61440 x 750 -- and a kernel of its own before this one: DESIGN.md.)
//
// Q(v) without a conversion: v 2^30 + 1.5 2^52 rounds v 2^30 to an integer in the add (ties to even,
// |v 2^30| < 2^51), and the sum's bit pattern is that of 1.5 2^52 plus the integer.  The LDS rows add
// the bit patterns; the flush takes count x bits(1.5 2^52) off again (mod 2^64, exact): every lane
// that adds to rows 1..3 of a slot adds one to row 0 of that slot.  The exception is slot numbins + 1
// (everything beyond r_max), where only rows 0 and 1 are added: hd needs 1 / r^2 (v_rcp_f64 and two
// Newton steps, relative error ~2^-50, against the 2^-31 the quantum allows), which is kept off the
// path of pairs beyond r_max together with p2 and two of the four atomics.
//
// Histograms: four 64-bit rows of numbins + 2 slots per wave in LDS, added to with workgroup-scope
// 64-bit LDS atomics, flushed to the global counters when the wave's replica changes (per-replica
// output), once per workgroup at the end (summed output).  |Q| <= 2^31 per pair and at most 2^41
// pairs per replica: the sums cannot wrap, no overflow flush.
#pragma once
#include "mmc_struct.hpp"

// MMC_ORIENT_MAX_BINS (include/mmc_hip.h): one wave per workgroup, thresholds 8 (numbins + 2) bytes and
// four 64-bit rows 32 (numbins + 2) bytes
static_assert(40 * (MMC_ORIENT_MAX_BINS + 2) <= TILE_LDS_BYTES && 40 * (MMC_ORIENT_MAX_BINS + 3) > TILE_LDS_BYTES,
              "MMC_ORIENT_MAX_BINS is what one wave fits");
#define OR_MAGIC 6755399441055744.0 // 1.5 2^52: x + OR_MAGIC has the bits of OR_MAGIC plus rint(x), |x| < 2^51
#define OR_MAGIC_BITS 0x4338000000000000ULL

struct OrientArgs {
    TileArgs ta;
    unsigned long long *hist; // [4][numbins + 2] or [R][4][numbins + 2], zeroed by the host
};

__device__ __forceinline__ unsigned long long or_quant(double v)
{
    return (unsigned long long)__double_as_longlong(v * MMC_ORIENT_SCALE + OR_MAGIC);
}

// Site 0 and the axis of molecule m of replica r: o[0..2] = site 0, o[3..5] = u.
template <bool REC>
__device__ __forceinline__ void or_molecule(const BatchView &bv, const double *__restrict__ rec, int r, int m,
                                            const BoxConsts &bc, double *o)
{
    const int f0 = bv.first0[m];
    const double q0 = bv.charge[f0], q1 = bv.charge[f0 + 1], q2 = bv.charge[f0 + 2];
    double t[12];
    load_sites12<REC>(bv, rec, r, m, t);
    double mu[3];
#pragma unroll
    for (int d = 0; d < 3; d++)
        mu[d] = (q0 * vector1D(t[9 + d], t[d], bc) + q1 * vector1D(t[9 + d], t[3 + d], bc))
                + q2 * vector1D(t[9 + d], t[6 + d], bc);
    const double n2 = (mu[0] * mu[0] + mu[1] * mu[1]) + mu[2] * mu[2];
    const bool ok = n2 > 0.0 && n2 < INFINITY; // (false for a NaN)
    const double n = sqrt(ok ? n2 : 1.0);
#pragma unroll
    for (int d = 0; d < 3; d++) {
        o[d] = t[d];
        o[3 + d] = ok ? mu[d] / n : 0.0;
    }
}

// REC: molecules are the 128-byte records of homogeneous batches; else the SoA arrays (load_sites12).
// grid and tiles: mmc_tiles.hpp.
template <bool REC>
__global__ __launch_bounds__(TILE_WAVES * 64) void k_orient_corr_wave(BatchView bv, const double *__restrict__ rec,
                                                                    OrientArgs oa)
{
    extern __shared__ __align__(16) unsigned char or_lds[];
    const TileArgs &ta = oa.ta;
    const int nb = ta.numbins, rs = nb + 2; // row stride: bins 0 .. numbins, then the slot beyond r_max
    const int tid = threadIdx.x, lane0 = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nw = (int)(blockDim.x >> 6);
    double *const thr = reinterpret_cast<double *>(or_lds);                                      // [rs]
    unsigned long long *const hall = reinterpret_cast<unsigned long long *>(or_lds + 8 * rs);    // [nw][4][rs]
    unsigned long long *const hw = hall + wv * 4 * rs;
    tile_prologue(thr, ta.thr, rs, hall, nw * 4 * rs);

    const int n_mol = bv.n_mol;
    const float inv_dr = ta.inv_dr, e_max = (float)(nb + 1);

    // counters src[n_src][4][rs] summed and added to dst[4][rs], the offsets of Q's bit patterns
    // taken off: n lanes added to rows 1..3 of a slot where row 0 of that slot counts n (rows 2 and
    // 3 of slot numbins + 1 are never added to)
    auto flush = [&](unsigned long long *dst, unsigned long long *src, int n_src, int first, int step, bool clear) {
        for (int q = first; q < rs; q += step) {
            unsigned long long v[4] = { 0ull, 0ull, 0ull, 0ull };
            for (int w = 0; w < n_src; w++)
#pragma unroll
                for (int row = 0; row < 4; row++)
                    v[row] += src[(w * 4 + row) * rs + q];
            if (v[0] != 0ull) {
                const unsigned long long off = v[0] * OR_MAGIC_BITS;
                atomicAdd(&dst[q], v[0]);
                atomicAdd(&dst[rs + q], v[1] - off);
                if (q <= nb) {
                    atomicAdd(&dst[2 * rs + q], v[2] - off);
                    atomicAdd(&dst[3 * rs + q], v[3] - off);
                }
            }
            if (clear)
#pragma unroll
                for (int row = 0; row < 4; row++)
                    src[row * rs + q] = 0ull;
        }
    };
    // this wave's counters added to dst and cleared
    auto flush_wave = [&](unsigned long long *dst) {
        wave_sync();
        flush(dst, hw, 1, lane0, 64, true);
        wave_sync();
    };

    TileCursor tc(ta, gridDim.x, blockIdx.x, nw, wv);
    if (tc.more()) {
        int r_hist = tc.r;
        double t[6]; // neighbour j: site 0, u
        BoxConsts bc = box_consts(bv.box);
        for (; tc.more(); tc.next()) {
            const int r = tc.r;
            // `lane` is made opaque once per unit (mmc_wave.hpp): lane-derived values are not hoisted
            // out of the persistent loop and held for the kernel's life
            int lane = lane0;
            asm volatile("" : "+v"(lane));
            if (ta.per_replica && r != r_hist) {
                flush_wave(oa.hist + (int64_t)r_hist * 4 * rs);
                r_hist = r;
            }
            const int j = 64 * tc.k + lane;
            if (tc.fresh) { // neighbour j of replica r (a lane beyond the last molecule loads the last)
                bc = box_consts(ta.box_r ? ta.box_r[r] : bv.box);
                or_molecule<REC>(bv, rec, r, min(j, n_mol - 1), bc, t);
                tc.fresh = false;
            }
            const double half = bc.half, neg_box = bc.neg;
            // the chosen molecules of block c: lane n computes molecule 64 c + n's six values, the
            // walk below reads them as wave-uniform values
            const int i_lo = 64 * tc.c, n_i = min(64, n_mol - i_lo);
            double cs[6];
            or_molecule<REC>(bv, rec, r, min(i_lo + lane, n_mol - 1), bc, cs);
            for (int ii = 0; ii < n_i; ii++) {
                const int i = i_lo + ii;
                const double sx = lane_f64(cs[0], ii), sy = lane_f64(cs[1], ii), sz = lane_f64(cs[2], ii);
                const double ux = lane_f64(cs[3], ii), uy = lane_f64(cs[4], ii), uz = lane_f64(cs[5], ii);
                const double xx = st_image(sx - t[0], half, neg_box);
                const double yy = st_image(sy - t[1], half, neg_box);
                const double zz = st_image(sz - t[2], half, neg_box);
                const double r2 = (xx * xx + yy * yy) + zz * zz;
                const int b = tile_bin(thr, r2, inv_dr, e_max);
                const double cc = (ux * t[3] + uy * t[4]) + uz * t[5];
                const bool pair = j > i && j < n_mol;
                if (pair) {
                    __hip_atomic_fetch_add(&hw[b], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_add(&hw[rs + b], or_quant(cc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                if (pair && b <= nb) {
                    const double ai = (ux * xx + uy * yy) + uz * zz;
                    const double aj = (t[3] * xx + t[4] * yy) + t[5] * zz;
                    double y = __builtin_amdgcn_rcp(r2); // 1 / r^2: two Newton steps on v_rcp_f64
                    y = fma(fma(-r2, y, 1.0), y, y);
                    y = fma(fma(-r2, y, 1.0), y, y);
                    const double hd = (r2 > 0.0) ? ((3.0 * ai) * aj) * y - cc : 0.0;
                    const double p2 = 1.5 * (cc * cc) - 0.5;
                    __hip_atomic_fetch_add(&hw[2 * rs + b], or_quant(hd), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_add(&hw[3 * rs + b], or_quant(p2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        if (ta.per_replica)
            flush_wave(oa.hist + (int64_t)r_hist * 4 * rs);
    }
    if (!ta.per_replica) { // once per workgroup: the waves' counters added up, then added to the total
        __syncthreads();
        flush(oa.hist, hall, nw, tid, (int)blockDim.x, false);
    }
}
