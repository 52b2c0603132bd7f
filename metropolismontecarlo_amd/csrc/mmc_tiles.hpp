// mmc_tiles.hpp -- what the pair passes over the i < j triangle share on the device:
// k_rdf_sites_wave (mmc_struct.hpp), k_orient_corr_wave (mmc_orient.hpp), k_pair_energy_wave
// (mmc_pair_energy.hpp) and k_sdf_wave (mmc_sdf.hpp, which gives the run of tiles to a workgroup and
// bins in three dimensions); the host side (tile_plan, tile_waves, obs_grid) is in mmc_units.inc.
//
// The decomposition.  The UNIT is a 64 x 64 tile (k, c), c <= k, of a replica's i < j triangle:
// neighbours j = 64 k + lane, chosen molecules i of block c.  A replica has K (K + 1) / 2 of them,
// K = ceil(n_mol / 64), numbered k-major; a launch has R times that many, replica-major.  The grid is
// any number of workgroups of blockDim.x / 64 waves, and wave W of NW takes the contiguous run
// [n_tiles W / NW, n_tiles (W + 1) / NW): tiles are equal work but for the half-masked diagonal ones,
// so a wave stays inside one or two replicas, and consecutive tiles of a wave keep (r, k), so the
// lane's neighbour is loaded once per row of tiles (`fresh`).  TileCursor walks the run; what a
// kernel keeps in registers per neighbour, its counters and when it flushes them are its own.
//
// The bin.  bin(r^2) = ceil(sqrt(r^2) / dr) is monotone in r^2, so the host builds, with that very
// fp64 arithmetic, thr[k] = the largest r^2 whose bin is <= k (mmc_units.inc: rdf_thresholds).  A
// float estimate e of the bin is within one of it (its relative error ~2e-7 is < 1e-3 bins at the
// 2046 bins allowed), and two compares against thr[e - 1], thr[e] (one ds_read2_b64) give the exact
// bin: thr[b - 1] < r^2 <= thr[b], without fp64 sqrt or divide.  Slot numbins + 1 of every row is
// where everything beyond r_max lands, so no lane branches on its bin.
#pragma once
#include "mmc_wave.hpp"

#define TILE_WAVES 4         // waves per workgroup (fewer where the counters would not fit: tile_waves)
#define TILE_LDS_BYTES 65536 // dynamic LDS a workgroup may ask for without opting in

struct TileArgs {
    const double *thr;     // [numbins + 2]: thr[k] = largest r^2 with bin <= k; thr[numbins + 1] = +inf
    const double *box_r;   // [R] per-replica boxes, or NULL: bv.box
    int32_t numbins, per_replica;
    float inv_dr;
    int32_t n_blocks;      // K = ceil(n_mol / 64)
    int32_t tiles_per_rep; // K (K + 1) / 2: tiles (k, c), c <= k, k-major
    int64_t n_tiles;       // R * tiles_per_rep
};

// The run of tiles of wave wv of the nw of workgroup `block` of `grid`, one tile at a time.
struct TileCursor {
    int64_t tile, end;
    int r, k, c, K;
    bool fresh; // (r, k) changed: the lane's neighbour is to be loaded (the kernel clears it)

    __device__ __forceinline__ TileCursor(const TileArgs &ta, unsigned grid, unsigned block, int nw, int wv)
        : TileCursor(ta, ta.n_tiles * ((int64_t)block * nw + wv) / ((int64_t)grid * nw),
                     ta.n_tiles * ((int64_t)block * nw + wv + 1) / ((int64_t)grid * nw))
    {
    }
    // ... or any run [first, last) of the launch's tiles (k_sdf_wave: a share of its workgroup's run)
    __device__ __forceinline__ TileCursor(const TileArgs &ta, int64_t first, int64_t last)
        : tile(first), end(last), r(0), k(0), c(0), K(ta.n_blocks), fresh(true)
    {
        if (tile < end) {
            const int T = ta.tiles_per_rep;
            r = (int)(tile / T);
            c = (int)(tile - (int64_t)r * T);
            while (c > k) { // tile index -> (k, c): rows of 1, 2, 3, ... tiles
                c -= k + 1;
                k++;
            }
        }
    }
    __device__ __forceinline__ bool more() const { return tile < end; }
    // the next tile: (k, c + 1), then the next row of tiles, then the next replica
    __device__ __forceinline__ void next()
    {
        tile++;
        if (++c > k) {
            c = 0;
            fresh = true;
            if (++k == K) {
                k = 0;
                r++;
            }
        }
    }
};

// The thresholds into LDS and n counter words of the workgroup zeroed, then the barrier.
template <class Word>
__device__ __forceinline__ void tile_prologue(double *thr, const double *__restrict__ src, int rs, Word *counters, int n)
{
    for (int q = threadIdx.x; q < rs; q += (int)blockDim.x)
        thr[q] = src[q];
    for (int q = threadIdx.x; q < n; q += (int)blockDim.x)
        counters[q] = 0;
    __syncthreads();
}

// The bin of r2 from the thresholds (in LDS): the float estimate, then the two compares.
__device__ __forceinline__ int tile_bin(const double *thr, double r2, float inv_dr, float e_max)
{
    float e = ceilf(__builtin_amdgcn_sqrtf((float)r2) * inv_dr);
    e = fminf(fmaxf(e, 1.0f), e_max); // 1 .. numbins + 1 (a NaN lands on 1: in bounds)
    int b = (int)e;
    const double lo = thr[b - 1], hi = thr[b];
    b += (r2 > hi) ? 1 : 0;
    b -= (r2 <= lo) ? 1 : 0;
    return b;
}

// The nine site coordinates of molecule m of replica r, t[3 a + d].  REC: from the 128-byte records
// of homogeneous batches (five 16-byte loads); else from the SoA arrays, slot a of molecule m at
// first0[m] + a (a batch holds three-atom molecules only).
template <bool REC>
__device__ __forceinline__ void load_sites9(const BatchView &bv, const double *__restrict__ rec, int r, int m, double *t)
{
    if constexpr (REC) {
        const double2 *src = reinterpret_cast<const double2 *>(rec + ((int64_t)r * bv.n_mol + m) * MMC_RSTRIDE);
        const double2 v0 = src[0], v1 = src[1], v2 = src[2], v3 = src[3], v4 = src[4];
        t[0] = v0.x; t[1] = v0.y; t[2] = v1.x; t[3] = v1.y; t[4] = v2.x; t[5] = v2.y;
        t[6] = v3.x; t[7] = v3.y; t[8] = v4.x;
    } else {
        const int64_t a0 = (int64_t)r * bv.atom_stride + bv.first0[m];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            t[3 * a] = bv.ax[a0 + a]; t[3 * a + 1] = bv.ay[a0 + a]; t[3 * a + 2] = bv.az[a0 + a];
        }
    }
}

// ... and with the centre of mass in t[9..11] (six 16-byte loads of the record).
template <bool REC>
__device__ __forceinline__ void load_sites12(const BatchView &bv, const double *__restrict__ rec, int r, int m, double *t)
{
    if constexpr (REC) {
        const double2 *src = reinterpret_cast<const double2 *>(rec + ((int64_t)r * bv.n_mol + m) * MMC_RSTRIDE);
#pragma unroll
        for (int q = 0; q < 6; q++) {
            const double2 v = src[q];
            t[2 * q] = v.x;
            t[2 * q + 1] = v.y;
        }
    } else {
        const int64_t mi = (int64_t)r * bv.mol_stride + m;
        load_sites9<false>(bv, rec, r, m, t);
        t[9] = bv.comx[mi]; t[10] = bv.comy[mi]; t[11] = bv.comz[mi];
    }
}
