// mmc_struct.hpp -- structure observables of every replica, read-only beside the chains:
//   k_rdf_sites_wave   the six site-site pair histograms of 3-site molecules in one pass
//   k_dipoles          the total dipole moment M_r = sum_i mu_i of every replica
//
// k_rdf_sites_wave keeps the pair loop of Ewald/gr.jl `makeRDF` (:68-92) for every atom-slot pair:
// the difference site(i) - site(j), i < j, its minimum image (:75-80: strict < -side/2 -> + side,
// > side/2 -> - side), r = sqrt((xx xx + yy yy) + zz zz) unfused, bin = ceil(r / dr), counted when
// bin <= numbins (:87-90).  Rows are the unordered slot pairs (0,0) (0,1) (0,2) (1,1) (1,2) (2,2);
// row (a,b), a < b, takes i.a - j.b and i.b - j.a.
//
// The scheme is k_move_eval_wave's (mmc_wave.hpp): a wavefront owns a unit and never waits for
// another wave inside it; lane n holds neighbour n's nine site coordinates in registers (five 16-byte
// loads of one 128-byte line), the chosen molecule's nine coordinates are scalar operands, all lanes
// work on the same atom pair.  The unit is a 64 x 64 tile of the i < j triangle and the bin comes
// from host-built thresholds: mmc_tiles.hpp has both, for this kernel and the two modelled on it.
// (Not k_total_wave's molecule pair (u, N-1-u): a unit of that kind gathers all N records for two
// chosen molecules, 36 MB of L2 traffic per 750-molecule replica where k_total_wave's COM gate
// gathers a fifth of them and this pass, which has no gate below L/2, would gather all.)  The 64
// neighbours of block k stay in registers while the wave walks the chosen molecules of block c <= k
// through scalar loads (issued outside the lane mask, before the previous molecule's nine binnings;
// scalar loads and LDS share a counter that can only be waited to zero, so the first threshold read
// of those binnings waits for the load too: its latency is hidden by the other resident waves, not
// by this one): the vector loads are one pass over the replica per row of tiles.
//
// Histograms are 32-bit, privatised per wave in LDS (6 rows x (numbins + 2)), flushed to the 64-bit
// global counters when the wave's replica changes (per-replica output), once per workgroup at the
// end (summed output) and before a counter could pass 2^31, bounded by the distances added since
// the last flush.  Counts are integers: the order of the flushes cannot change them.
#pragma once
#include "mmc_tiles.hpp"

#define ST_WAVES 4            // waves per workgroup of k_dipoles
#define MMC_RDF_SITES_MAX_BINS 2046 // one wave per workgroup: 32 (numbins + 2) bytes
#define ST_TILE_DIST (64u * 64u * 9u) // no counter gains more than this in one tile

struct RdfSitesArgs {
    TileArgs ta;
    unsigned long long *hist; // [6][numbins + 1] or [R][6][numbins + 1], zeroed by the host
};

// gr.jl:75-80 on one component: |d| > side/2 (strict on both sides) moves d by one side.  -side m
// is exact, so the fma rounds d -+ side once, as the reference's addition does.
__device__ __forceinline__ double st_image(double d, double half, double neg_box)
{
    const double m = (fabs(d) > half) ? copysign(1.0, d) : 0.0;
    return fma(m, neg_box, d);
}

__device__ __forceinline__ void st_count(unsigned *row, const double *thr, double xx, double yy, double zz,
                                         float inv_dr, float e_max)
{
    const int b = tile_bin(thr, (xx * xx + yy * yy) + zz * zz, inv_dr, e_max);
    __hip_atomic_fetch_add(&row[b], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// REC: molecules are the 128-byte records of homogeneous batches; else the SoA arrays (load_sites9).
// grid and tiles: mmc_tiles.hpp.
template <bool REC>
__global__ __launch_bounds__(TILE_WAVES * 64) void k_rdf_sites_wave(BatchView bv, const double *__restrict__ rec,
                                                                    RdfSitesArgs sa)
{
    extern __shared__ __align__(16) unsigned char st_lds[];
    const TileArgs &ta = sa.ta;
    const int nb = ta.numbins, rs = nb + 2; // row stride: bins 0 .. numbins, then the slot beyond r_max
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nw = (int)(blockDim.x >> 6);
    double *const thr = reinterpret_cast<double *>(st_lds);                 // [rs]
    unsigned *const hall = reinterpret_cast<unsigned *>(st_lds + 8 * rs);   // [nw][6][rs]
    unsigned *const hw = hall + wv * 6 * rs;
    tile_prologue(thr, ta.thr, rs, hall, nw * 6 * rs);

    const int n_mol = bv.n_mol;
    const float inv_dr = ta.inv_dr, e_max = (float)(nb + 1);
    const int64_t row_len = nb + 1;

    // this wave's counters added to dst[6][numbins + 1] and cleared
    auto flush_wave = [&](unsigned long long *dst) {
        wave_sync();
        for (int q = lane; q < 6 * rs; q += 64) {
            const int row = q / rs, bin = q - row * rs;
            const unsigned v = hw[q];
            if (v != 0u && bin <= nb)
                atomicAdd(&dst[row * row_len + bin], (unsigned long long)v);
            hw[q] = 0u;
        }
        wave_sync();
    };

    TileCursor tc(ta, gridDim.x, blockIdx.x, nw, wv);
    if (tc.more()) {
        int r_hist = tc.r;
        unsigned since = 0u; // distances a counter may have gained since the last flush
        double t[9];
        double half = 0.0, neg_box = 0.0;
        for (; tc.more(); tc.next()) {
            const int r = tc.r;
            if (ta.per_replica && r != r_hist) {
                flush_wave(sa.hist + (int64_t)r_hist * 6 * row_len);
                r_hist = r;
                since = 0u;
            }
            if (since > 0x7fffffffu - ST_TILE_DIST) {
                flush_wave(sa.hist + (ta.per_replica ? (int64_t)r_hist * 6 * row_len : 0));
                since = 0u;
            }
            since += ST_TILE_DIST;
            const int j = 64 * tc.k + lane;
            if (tc.fresh) { // neighbour j of replica r (a lane beyond the last molecule loads the last)
                load_sites9<REC>(bv, rec, r, min(j, n_mol - 1), t);
                const double box = ta.box_r ? ta.box_r[r] : bv.box;
                half = box / 2.0;
                neg_box = -box;
                tc.fresh = false;
            }
            // the chosen molecules i of block c, one after the other: nine wave-uniform coordinates
            const int i_lo = 64 * tc.c, i_hi = min(i_lo + 64, n_mol);
            double nx[9];
            load_sites9<REC>(bv, rec, r, i_lo, nx);
            for (int i = i_lo; i < i_hi; i++) {
                double s[9];
#pragma unroll
                for (int q = 0; q < 9; q++)
                    s[q] = nx[q];
                // issued outside the lane mask (see the header on its latency)
                load_sites9<REC>(bv, rec, r, min(i + 1, n_mol - 1), nx);
                if (j > i && j < n_mol) {
#pragma unroll
                    for (int a = 0; a < 3; a++) {
#pragma unroll
                        for (int bq = 0; bq < 3; bq++) {
                            const int row = a <= bq ? (a == 0 ? bq : a + bq + 1) : (bq == 0 ? a : a + bq + 1);
                            const double xx = st_image(s[3 * a] - t[3 * bq], half, neg_box);
                            const double yy = st_image(s[3 * a + 1] - t[3 * bq + 1], half, neg_box);
                            const double zz = st_image(s[3 * a + 2] - t[3 * bq + 2], half, neg_box);
                            st_count(hw + row * rs, thr, xx, yy, zz, inv_dr, e_max);
                        }
                    }
                }
            }
        }
        if (ta.per_replica)
            flush_wave(sa.hist + (int64_t)r_hist * 6 * row_len);
    }
    if (!ta.per_replica) { // once per workgroup: the waves' counters added up, then added to the total
        __syncthreads();
        for (int q = tid; q < 6 * rs; q += (int)blockDim.x) {
            const int row = q / rs, bin = q - row * rs;
            unsigned long long v = 0;
            for (int w = 0; w < nw; w++)
                v += hall[w * 6 * rs + q];
            if (v != 0 && bin <= nb)
                atomicAdd(&sa.hist[row * row_len + bin], v);
        }
    }
}

// One wave per replica: lane l adds mu_i of molecules i = l, l + 64, ... in that order, then the 64
// lane sums are added by wave_sum_rows (DPP, fixed order): the bits do not depend on the launch.
// mu_i = (q_0 d_0 + q_1 d_1) + q_2 d_2 (+ ... for longer molecules) per component, unfused, d_a the
// minimum image (vector1D, boundaries.jl) of atom a minus the molecule's centre of mass.
template <bool REC>
__global__ __launch_bounds__(ST_WAVES * 64) void k_dipoles(BatchView bv, const double *__restrict__ rec,
                                                           const double *__restrict__ box_r, double *dip, int R)
{
    const int lane = threadIdx.x & 63;
    const int r = (int)blockIdx.x * ST_WAVES + (int)(threadIdx.x >> 6);
    if (r >= R)
        return;
    const BoxConsts bc = box_consts(box_r ? box_r[r] : bv.box);
    const int n_mol = bv.n_mol;
    double acc[3] = { 0.0, 0.0, 0.0 };
    for (int i = lane; i < n_mol; i += 64) {
        const int f0 = bv.first0[i];
        double mu[3];
        if constexpr (REC) {
            double t[12];
            load_sites12<true>(bv, rec, r, i, t);
            const double q0 = bv.charge[f0], q1 = bv.charge[f0 + 1], q2 = bv.charge[f0 + 2];
#pragma unroll
            for (int d = 0; d < 3; d++)
                mu[d] = (q0 * vector1D(t[9 + d], t[d], bc) + q1 * vector1D(t[9 + d], t[3 + d], bc))
                        + q2 * vector1D(t[9 + d], t[6 + d], bc);
        } else {
            const int64_t m = (int64_t)r * bv.mol_stride + i, a0 = (int64_t)r * bv.atom_stride + f0;
            const double cx = bv.comx[m], cy = bv.comy[m], cz = bv.comz[m];
            const int na = bv.cnt[i];
            mu[0] = mu[1] = mu[2] = 0.0;
            for (int a = 0; a < na; a++) {
                const double q = bv.charge[f0 + a];
                const double px = q * vector1D(cx, bv.ax[a0 + a], bc), py = q * vector1D(cy, bv.ay[a0 + a], bc),
                             pz = q * vector1D(cz, bv.az[a0 + a], bc);
                mu[0] = a ? mu[0] + px : px;
                mu[1] = a ? mu[1] + py : py;
                mu[2] = a ? mu[2] + pz : pz;
            }
        }
        acc[0] += mu[0];
        acc[1] += mu[1];
        acc[2] += mu[2];
    }
    const double s0 = wave_sum_rows(acc[0]), s1 = wave_sum_rows(acc[1]), s2 = wave_sum_rows(acc[2]);
    if (lane == 0) {
        dip[3 * (int64_t)r] = s0;
        dip[3 * (int64_t)r + 1] = s1;
        dip[3 * (int64_t)r + 2] = s2;
    }
}
