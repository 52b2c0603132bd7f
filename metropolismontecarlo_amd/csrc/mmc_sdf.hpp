// mmc_sdf.hpp -- spatial distribution functions of every replica, read-only beside the chains:
//   k_sdf_wave   counts of the neighbours' sites per cell of a cube in the body-fixed frame of the
//                centre molecule, every pair i < j deposited both ways (include/mmc_hip.h, "Spatial
//                distribution functions"; restated in numpy by tests/sdf_ref.py)
//
// The walk is k_orient_corr_wave's (mmc_orient.hpp) on mmc_tiles.hpp's tiles.  Lane n keeps neighbour
// n of block k across a row of tiles -- eighteen doubles: site 0, the three axes and the offsets of
// sites 1 and 2 -- computed once per (replica, block) by the lane that loads the record (a square
// root and three divisions per axis).  At the start of a tile the 64 lanes compute block c's
// eighteen as well, and the walk over the chosen molecules pulls them out with v_readlane, so the
// pair loop has no memory load.  A pair makes two deposits per selected site: the neighbour's site
// in the chosen molecule's frame (scalar axes, the lane's vector) and the chosen molecule's site in
// the neighbour's frame (the lane's axes, -d bit for bit plus a scalar offset).
//
// The cell.  Along an axis the cell of p is k with e_k <= p < e_k+1, e_k = (double)k * cell, which
// the host builds with that very multiplication (edge[k + n_half], k = -n_half .. n_half, in LDS).
// A float estimate floor((float)p / cell) is within one of it (relative error ~2e-7 against at most
// 25 cells a side), clamped to the axis' cells; two compares against edge[q], edge[q + 1] (one
// ds_read2_b64) correct it, and carry a p beyond the cube to -1 or n: no lane branches on its cell.
// A NaN is clamped to the lowest cell (fmaxf returns its other operand) and fails `p >= lo`: -1.
// A folded axis takes |p| and the upper half of the same edges.  Deposits outside the cube, and those
// of a centre without a frame, are counted by ballot in scalar registers: only deposits inside reach
// the LDS atomic (64 lanes adding to one spare slot would serialise).
//
// Counters: ONE grid of 32-bit words per workgroup in LDS, shared by all its waves (up to 128 KB: a
// grid per wave does not fit), added to with workgroup-scope LDS atomics, its non-zero cells flushed
// with 64-bit global atomics.  Two things follow from sharing it:
//   per-replica output -- the run of tiles belongs to the WORKGROUP (mmc_tiles.hpp's split with the
//     workgroup in the wave's place), is cut into segments where the replica changes, the waves
//     share a segment's tiles (contiguous shares, so a wave still keeps its neighbour along a row of
//     tiles) and meet at a barrier and a flush after each;
//   overflow -- a segment is cut after SDF_FLUSH_TILES tiles at the latest, whatever the output: a
//     tile makes at most 64 x 64 x 2 x 3 deposits, all of which may fall into one cell.
// All counts are integers: no grid, "wave_wgs", flush order or order of atomics changes a bit.
#pragma once
#include "mmc_tiles.hpp"

#define SDF_THREADS 1024        // the largest workgroup: 16 waves, 4 per SIMD, at most 128 VGPRs a lane
#define SDF_FLUSH_TILES 131072  // tiles of a workgroup between two flushes of its grid
static_assert((unsigned long long)SDF_FLUSH_TILES * 64 * 64 * 2 * 3 < (1ull << 32),
              "a 32-bit cell of the workgroup's grid cannot wrap between two flushes");
// MMC_SDF_MAX_CELLS (include/mmc_hip.h): 32-bit cells in 128 KB of the 160 KB a gfx950 workgroup may
// claim; the edges (at most 2 x 25 + 1 doubles) and the scaffold beside them
static_assert(4 * MMC_SDF_MAX_CELLS == 131072, "MMC_SDF_MAX_CELLS is what 128 KB of LDS hold");

struct SdfArgs {
    TileArgs ta;               // (thr: the 2 n_half + 1 edges; numbins and inv_dr unused)
    unsigned long long *hist;  // [cells + 2] or [R][cells + 2], zeroed by the host
    int32_t n_half, fold, site_mask;
    int32_t n_cells;           // g_x g_y g_z
    float inv_cell;
};

// One axis of the grid: cells k_min .. k_min + n - 1, their edges from edge[off].
struct SdfAxis {
    int off, n;
    float lo, hi; // k_min, k_min + n - 1
    unsigned abs_mask; // and-mask of p's high dword: 0x7fffffff folds
};
__device__ __forceinline__ SdfAxis sd_axis(int n_half, bool folded)
{
    SdfAxis a;
    a.off = folded ? n_half : 0;
    a.n = folded ? n_half : 2 * n_half;
    a.lo = folded ? 0.0f : -(float)n_half;
    a.hi = (float)(n_half - 1);
    a.abs_mask = folded ? 0x7fffffffu : 0xffffffffu;
    return a;
}

// The cell of p along an axis, 0 .. n - 1; -1 or n beyond the cube (-1 for a NaN).
__device__ __forceinline__ int sd_cell(const double *edge, const SdfAxis &ax, double p, float inv_cell)
{
    const long long bits = __double_as_longlong(p);
    p = __longlong_as_double((bits & 0xffffffffll) | ((long long)((unsigned)(bits >> 32) & ax.abs_mask) << 32));
    float e = floorf((float)p * inv_cell);
    e = fminf(fmaxf(e, ax.lo), ax.hi);
    int q = (int)e - (int)ax.lo;
    const double lo = edge[ax.off + q], hi = edge[ax.off + q + 1];
    q -= (p >= lo) ? 0 : 1;
    q += (p >= hi) ? 1 : 0;
    return q;
}

struct SdfGrid {
    unsigned *cells;    // the workgroup's grid in LDS
    const double *edge; // [2 n_half + 1] in LDS
    SdfAxis x, y, z;
    float inv_cell;
};

// One deposit of each lane with `on`: the cell of (px, py, pz) counted, or `outside`.
__device__ __forceinline__ void sd_deposit(const SdfGrid &g, double px, double py, double pz, bool on,
                                           unsigned long long &outside)
{
    const int ix = sd_cell(g.edge, g.x, px, g.inv_cell);
    const int iy = sd_cell(g.edge, g.y, py, g.inv_cell);
    const int iz = sd_cell(g.edge, g.z, pz, g.inv_cell);
    const bool in = (unsigned)ix < (unsigned)g.x.n && (unsigned)iy < (unsigned)g.y.n && (unsigned)iz < (unsigned)g.z.n;
    if (on && in)
        __hip_atomic_fetch_add(&g.cells[(ix * g.y.n + iy) * g.z.n + iz], 1u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
    outside += (unsigned long long)__popcll(__ballot(on && !in));
}

__device__ __forceinline__ double sd_dot(double ax, double ay, double az, double bx, double by, double bz)
{
    return (ax * bx + ay * by) + az * bz;
}

// Molecule m of replica r: o[0..2] site 0, o[3..5] e_x, o[6..8] e_y, o[9..11] e_z, o[12..14] o_1,
// o[15..17] o_2.  Returns whether it has a frame (the axes are then finite unit vectors).
template <bool REC>
__device__ __forceinline__ bool sd_molecule(const BatchView &bv, const double *__restrict__ rec, int r, int m,
                                            const BoxConsts &bc, double *o)
{
    double t[9];
    load_sites9<REC>(bv, rec, r, m, t);
    double b[3], h[3], ez[3], g[3], ex[3];
#pragma unroll
    for (int d = 0; d < 3; d++) {
        o[d] = t[d];
        o[12 + d] = vector1D(t[d], t[3 + d], bc);
        o[15 + d] = vector1D(t[d], t[6 + d], bc);
        b[d] = o[12 + d] + o[15 + d];
        h[d] = o[15 + d] - o[12 + d];
    }
    const double nb2 = sd_dot(b[0], b[1], b[2], b[0], b[1], b[2]);
    const double nb = sqrt(nb2);
#pragma unroll
    for (int d = 0; d < 3; d++)
        ez[d] = b[d] / nb;
    const double tt = sd_dot(h[0], h[1], h[2], ez[0], ez[1], ez[2]);
#pragma unroll
    for (int d = 0; d < 3; d++)
        g[d] = h[d] - tt * ez[d];
    const double ng2 = sd_dot(g[0], g[1], g[2], g[0], g[1], g[2]);
    const double ng = sqrt(ng2);
#pragma unroll
    for (int d = 0; d < 3; d++)
        ex[d] = g[d] / ng;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const int d1 = (d + 1) % 3, d2 = (d + 2) % 3;
        o[3 + d] = ex[d];
        o[6 + d] = ez[d1] * ex[d2] - ez[d2] * ex[d1];
        o[9 + d] = ez[d];
    }
    return nb2 > 0.0 && nb2 < INFINITY && ng2 > 0.0 && ng2 < INFINITY; // (false for a NaN)
}

// REC: molecules are the 128-byte records of homogeneous batches; else the SoA arrays (load_sites9).
// Any grid of workgroups of any number of waves; dynamic LDS: the edges, then n_cells words.
template <bool REC>
__global__ __launch_bounds__(SDF_THREADS) void k_sdf_wave(BatchView bv, const double *__restrict__ rec, SdfArgs sa)
{
    extern __shared__ __align__(16) unsigned char sd_lds[];
    const TileArgs &ta = sa.ta;
    const int n_edge = 2 * sa.n_half + 1, n_cells = sa.n_cells;
    const int tid = threadIdx.x, lane0 = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nw = (int)(blockDim.x >> 6);
    double *const edge = reinterpret_cast<double *>(sd_lds);
    SdfGrid g;
    g.cells = reinterpret_cast<unsigned *>(sd_lds + 8 * n_edge);
    g.edge = edge;
    g.x = sd_axis(sa.n_half, (sa.fold & 1) != 0);
    g.y = sd_axis(sa.n_half, (sa.fold & 2) != 0);
    g.z = sd_axis(sa.n_half, false);
    g.inv_cell = sa.inv_cell;
    tile_prologue(edge, ta.thr, n_edge, g.cells, n_cells);

    const int n_mol = bv.n_mol;
    const bool sel0 = (sa.site_mask & 1) != 0, sel1 = (sa.site_mask & 2) != 0, sel2 = (sa.site_mask & 4) != 0;
    const unsigned n_sel = (unsigned)__popc((unsigned)sa.site_mask);
    const int64_t row_len = (int64_t)n_cells + 2;

    // the workgroup's run of tiles, a segment at a time: to the next replica (per-replica output), to
    // SDF_FLUSH_TILES tiles, or to the end of the run
    int64_t t0 = ta.n_tiles * (int64_t)blockIdx.x / (int64_t)gridDim.x;
    const int64_t t1 = ta.n_tiles * ((int64_t)blockIdx.x + 1) / (int64_t)gridDim.x;
    while (t0 < t1) {
        int64_t seg_end = min(t1, t0 + (int64_t)SDF_FLUSH_TILES);
        unsigned long long *dst = sa.hist;
        if (ta.per_replica) {
            const int64_t r_seg = t0 / ta.tiles_per_rep;
            seg_end = min(seg_end, (r_seg + 1) * ta.tiles_per_rep);
            dst += r_seg * row_len;
        }
        const int64_t len = seg_end - t0;
        unsigned long long outside = 0ull, noframe = 0ull; // of this wave, in scalar registers

        double t[18]; // neighbour j
        bool fj = false;
        BoxConsts bc = box_consts(bv.box);
        for (TileCursor tc(ta, t0 + len * wv / nw, t0 + len * (wv + 1) / nw); tc.more(); tc.next()) {
            const int r = tc.r;
            // `lane` is made opaque once per unit (mmc_wave.hpp): lane-derived values are not hoisted
            // out of the persistent loop and held for the kernel's life
            int lane = lane0;
            asm volatile("" : "+v"(lane));
            const int j = 64 * tc.k + lane;
            if (tc.fresh) { // neighbour j of replica r (a lane beyond the last molecule loads the last)
                bc = box_consts(ta.box_r ? ta.box_r[r] : bv.box);
                fj = sd_molecule<REC>(bv, rec, r, min(j, n_mol - 1), bc, t);
                tc.fresh = false;
            }
            // the chosen molecules of block c: lane n computes molecule 64 c + n's eighteen values,
            // the walk below reads them as wave-uniform values
            const int i_lo = 64 * tc.c, n_i = min(64, n_mol - i_lo);
            double cs[18];
            const unsigned long long fc = __ballot(sd_molecule<REC>(bv, rec, r, min(i_lo + lane, n_mol - 1), bc, cs));
            for (int ii = 0; ii < n_i; ii++) {
                const int i = i_lo + ii;
                const bool pair = j > i && j < n_mol;
                const bool fi = ((fc >> ii) & 1ull) != 0ull;
                // d = vector1D(site 0 of i, site 0 of j)
                const double dx = vector1D(lane_f64(cs[0], ii), t[0], bc);
                const double dy = vector1D(lane_f64(cs[1], ii), t[1], bc);
                const double dz = vector1D(lane_f64(cs[2], ii), t[2], bc);
                const unsigned n_pair = (unsigned)__popcll(__ballot(pair));
                // into i's frame: the lane's vector on scalar axes
                if (!fi) {
                    noframe += (unsigned long long)(n_pair * n_sel);
                } else {
                    const double exx = lane_f64(cs[3], ii), exy = lane_f64(cs[4], ii), exz = lane_f64(cs[5], ii);
                    const double eyx = lane_f64(cs[6], ii), eyy = lane_f64(cs[7], ii), eyz = lane_f64(cs[8], ii);
                    const double ezx = lane_f64(cs[9], ii), ezy = lane_f64(cs[10], ii), ezz = lane_f64(cs[11], ii);
                    auto into_i = [&](double wx, double wy, double wz) {
                        sd_deposit(g, sd_dot(exx, exy, exz, wx, wy, wz), sd_dot(eyx, eyy, eyz, wx, wy, wz),
                                   sd_dot(ezx, ezy, ezz, wx, wy, wz), pair, outside);
                    };
                    if (sel0)
                        into_i(dx, dy, dz);
                    if (sel1)
                        into_i(dx + t[12], dy + t[13], dz + t[14]);
                    if (sel2)
                        into_i(dx + t[15], dy + t[16], dz + t[17]);
                }
                // into j's frame: -d plus i's scalar offset on the lane's axes
                noframe += (unsigned long long)((unsigned)__popcll(__ballot(pair && !fj)) * n_sel);
                auto into_j = [&](double wx, double wy, double wz) {
                    sd_deposit(g, sd_dot(t[3], t[4], t[5], wx, wy, wz), sd_dot(t[6], t[7], t[8], wx, wy, wz),
                               sd_dot(t[9], t[10], t[11], wx, wy, wz), pair && fj, outside);
                };
                if (sel0)
                    into_j(-dx, -dy, -dz);
                if (sel1)
                    into_j(-dx + lane_f64(cs[12], ii), -dy + lane_f64(cs[13], ii), -dz + lane_f64(cs[14], ii));
                if (sel2)
                    into_j(-dx + lane_f64(cs[15], ii), -dy + lane_f64(cs[16], ii), -dz + lane_f64(cs[17], ii));
            }
        }

        // the segment's counts added to its output, and the grid cleared for the next
        __syncthreads();
        for (int q = tid; q < n_cells; q += (int)blockDim.x) {
            const unsigned v = g.cells[q];
            if (v != 0u) {
                atomicAdd(&dst[q], (unsigned long long)v);
                g.cells[q] = 0u;
            }
        }
        if (lane0 == 0) {
            if (outside != 0ull)
                atomicAdd(&dst[n_cells], outside);
            if (noframe != 0ull)
                atomicAdd(&dst[n_cells + 1], noframe);
        }
        __syncthreads();
        t0 = seg_end;
    }
}
