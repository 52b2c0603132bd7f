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
// another wave inside it; lane n holds neighbour n's whole record in registers (six 16-byte loads
// of one 128-byte line), the chosen molecule's nine coordinates are scalar operands, all lanes work
// on the same atom pair.  The UNIT is a 64 x 64 tile of the i < j triangle, not k_total_wave's
// molecule pair (u, N-1-u): a unit of that kind gathers all N records for two chosen molecules,
// 36 MB of L2 traffic per 750-molecule replica where k_total_wave's COM gate gathers a fifth of
// them and this pass, which has no gate below L/2, would gather all.  Here the 64 neighbours of
// block k stay in registers while the wave walks the chosen molecules of block c <= k through
// scalar loads (issued outside the lane mask, before the previous molecule's nine binnings; scalar
// loads and LDS share a counter that can only be waited to zero, so the first threshold read of
// those binnings waits for the load too: its latency is hidden by the other resident waves, not by
// this one), and consecutive tiles of a
// wave keep k: the vector loads are one pass over the replica per row of tiles.  Tiles are equal
// work but for the half-masked diagonal ones, and a wave takes a contiguous run of them, so it
// stays inside one or two replicas.
//
// The bin is found without fp64 sqrt or divide: bin(r^2) = ceil(sqrt(r^2) / dr) is monotone in
// r^2, so the host builds, with that very fp64 arithmetic, thr[k] = the largest r^2 whose bin is
// <= k (mmc_struct.inc: rdf_thresholds).  A float estimate e of the bin is within one of it (its
// relative error ~2e-7 is < 1e-3 bins at the 2046 bins allowed), and two compares against
// thr[e - 1], thr[e] (one ds_read2_b64) give the exact bin: thr[b - 1] < r^2 <= thr[b].  Slot
// numbins + 1 of every row is where everything beyond r_max lands, so no lane branches on its bin.
//
// Histograms are 32-bit, privatised per wave in LDS (6 rows x (numbins + 2)), flushed to the 64-bit
// global counters when the wave's replica changes (per-replica output), once per workgroup at the
// end (summed output) and before a counter could pass 2^31, bounded by the distances added since
// the last flush.  Counts are integers: the order of the flushes cannot change them.
#pragma once
#include "mmc_wave.hpp"

#define ST_WAVES 4            // waves per workgroup (fewer where the histograms would not fit: host)
#define ST_LDS_BYTES 65536    // dynamic LDS a workgroup may ask for without opting in
#define MMC_RDF_SITES_MAX_BINS 2046 // one wave per workgroup: 32 (numbins + 2) bytes
#define ST_TILE_DIST (64u * 64u * 9u) // no counter gains more than this in one tile

struct RdfSitesArgs {
    const double *thr;        // [numbins + 2]: thr[k] = largest r^2 with bin <= k; thr[numbins + 1] = +inf
    const double *box_r;      // [R] per-replica boxes, or NULL: bv.box
    unsigned long long *hist; // [6][numbins + 1] or [R][6][numbins + 1], zeroed by the host
    int32_t numbins, per_replica;
    float inv_dr;
    int32_t n_blocks;         // K = ceil(n_mol / 64)
    int32_t tiles_per_rep;    // K (K + 1) / 2: tiles (k, c), c <= k, k-major
    int64_t n_tiles;          // R * tiles_per_rep
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
    const double r2 = (xx * xx + yy * yy) + zz * zz;
    float e = ceilf(__builtin_amdgcn_sqrtf((float)r2) * inv_dr);
    e = fminf(fmaxf(e, 1.0f), e_max); // 1 .. numbins + 1 (a NaN lands on 1: in bounds)
    int b = (int)e;
    const double lo = thr[b - 1], hi = thr[b];
    b += (r2 > hi) ? 1 : 0;
    b -= (r2 <= lo) ? 1 : 0;
    __hip_atomic_fetch_add(&row[b], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// REC: molecules are the 128-byte records of homogeneous batches; else the SoA arrays, slot a of
// molecule j at first0[j] + a (a batch holds three-atom molecules only).
// grid: any number of workgroups of blockDim.x / 64 waves; wave W of NW takes tiles
// [n_tiles W / NW, n_tiles (W + 1) / NW).
template <bool REC>
__global__ __launch_bounds__(ST_WAVES * 64) void k_rdf_sites_wave(BatchView bv, const double *__restrict__ rec,
                                                                  RdfSitesArgs sa)
{
    extern __shared__ __align__(16) unsigned char st_lds[];
    const int nb = sa.numbins, rs = nb + 2; // row stride: bins 0 .. numbins, then the slot beyond r_max
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nw = (int)(blockDim.x >> 6);
    double *const thr = reinterpret_cast<double *>(st_lds);                 // [rs]
    unsigned *const hall = reinterpret_cast<unsigned *>(st_lds + 8 * rs);   // [nw][6][rs]
    unsigned *const hw = hall + wv * 6 * rs;
    for (int q = tid; q < rs; q += (int)blockDim.x)
        thr[q] = sa.thr[q];
    for (int q = tid; q < nw * 6 * rs; q += (int)blockDim.x)
        hall[q] = 0u;
    __syncthreads();

    const int n_mol = bv.n_mol, K = sa.n_blocks, T = sa.tiles_per_rep;
    const float inv_dr = sa.inv_dr, e_max = (float)(nb + 1);
    const int64_t NW = (int64_t)gridDim.x * nw, W = (int64_t)blockIdx.x * nw + wv;
    const int64_t t0 = sa.n_tiles * W / NW, t1 = sa.n_tiles * (W + 1) / NW;
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

    if (t0 < t1) {
        int r = (int)(t0 / T), k = 0, c = (int)(t0 - (int64_t)r * T);
        while (c > k) { // tile index -> (k, c): rows of 1, 2, 3, ... tiles
            c -= k + 1;
            k++;
        }
        int r_hist = r;
        unsigned since = 0u; // distances a counter may have gained since the last flush
        bool fresh = true;   // (r, k) changed: the lane's neighbour record is to be loaded
        double t[9];
        double half = 0.0, neg_box = 0.0;
        for (int64_t tile = t0; tile < t1; tile++) {
            if (sa.per_replica && r != r_hist) {
                flush_wave(sa.hist + (int64_t)r_hist * 6 * row_len);
                r_hist = r;
                since = 0u;
            }
            if (since > 0x7fffffffu - ST_TILE_DIST) {
                flush_wave(sa.hist + (sa.per_replica ? (int64_t)r_hist * 6 * row_len : 0));
                since = 0u;
            }
            since += ST_TILE_DIST;
            const int j = 64 * k + lane;
            if (fresh) { // neighbour j of replica r (a lane beyond the last molecule loads the last)
                const int jc = min(j, n_mol - 1);
                if constexpr (REC) {
                    const double2 *src = reinterpret_cast<const double2 *>(rec + ((int64_t)r * n_mol + jc) * MMC_RSTRIDE);
                    const double2 v0 = src[0], v1 = src[1], v2 = src[2], v3 = src[3], v4 = src[4];
                    t[0] = v0.x; t[1] = v0.y; t[2] = v1.x; t[3] = v1.y; t[4] = v2.x; t[5] = v2.y;
                    t[6] = v3.x; t[7] = v3.y; t[8] = v4.x;
                } else {
                    const int64_t a0 = (int64_t)r * bv.atom_stride + bv.first0[jc];
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        t[3 * a] = bv.ax[a0 + a]; t[3 * a + 1] = bv.ay[a0 + a]; t[3 * a + 2] = bv.az[a0 + a];
                    }
                }
                const double box = sa.box_r ? sa.box_r[r] : bv.box;
                half = box / 2.0;
                neg_box = -box;
                fresh = false;
            }
            // the chosen molecules i of block c, one after the other: nine wave-uniform coordinates
            const int i_lo = 64 * c, i_hi = min(i_lo + 64, n_mol);
            auto chosen = [&](int i, double *o) {
                if constexpr (REC) {
                    const double *p = rec + ((int64_t)r * n_mol + i) * MMC_RSTRIDE;
#pragma unroll
                    for (int q = 0; q < 9; q++)
                        o[q] = p[q];
                } else {
                    const int64_t a0 = (int64_t)r * bv.atom_stride + bv.first0[i];
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        o[3 * a] = bv.ax[a0 + a]; o[3 * a + 1] = bv.ay[a0 + a]; o[3 * a + 2] = bv.az[a0 + a];
                    }
                }
            };
            double nx[9];
            chosen(i_lo, nx);
            for (int i = i_lo; i < i_hi; i++) {
                double s[9];
#pragma unroll
                for (int q = 0; q < 9; q++)
                    s[q] = nx[q];
                chosen(min(i + 1, n_mol - 1), nx); // issued outside the lane mask (see the header on its latency)
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
            // the next tile: (k, c + 1), then the next row of tiles, then the next replica
            if (++c > k) {
                c = 0;
                fresh = true;
                if (++k == K) {
                    k = 0;
                    r++;
                }
            }
        }
        if (sa.per_replica)
            flush_wave(sa.hist + (int64_t)r_hist * 6 * row_len);
    }
    if (!sa.per_replica) { // once per workgroup: the waves' counters added up, then added to the total
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
            const double2 *src = reinterpret_cast<const double2 *>(rec + ((int64_t)r * n_mol + i) * MMC_RSTRIDE);
            double t[MMC_REC];
#pragma unroll
            for (int q = 0; q < 6; q++) {
                const double2 v = src[q];
                t[2 * q] = v.x;
                t[2 * q + 1] = v.y;
            }
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
