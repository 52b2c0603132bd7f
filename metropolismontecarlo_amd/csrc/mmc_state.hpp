// mmc_state.hpp -- the state record of one replica (include/mmc_hip.h, "Save and resume"): its layout,
// a pure host function, and the two kernels that pack records from and unpack them into every layout
// the batch keeps.  The layout half needs no HIP, so a host-only program can include this file.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct StateLayout {
    int64_t off[8]; // box, temperature, flags, com, coords, S, quat, end of the data
    int64_t bytes;  // of a record: a multiple of 64
};

// Sections start on 16 bytes, so that both kernels move 16 bytes per lane throughout.
static inline StateLayout state_layout(int64_t n_mol, int64_t nkvecs, bool quat)
{
    auto up = [](int64_t x, int64_t a) { return (x + a - 1) / a * a; };
    StateLayout L;
    L.off[0] = 0;
    L.off[1] = 8;
    L.off[2] = 16;
    L.off[3] = 32;
    L.off[4] = up(L.off[3] + 24 * n_mol, 16);
    L.off[5] = up(L.off[4] + 72 * n_mol, 16);
    L.off[6] = up(L.off[5] + 16 * nkvecs, 16);
    L.off[7] = L.off[6] + (quat ? 32 * n_mol : 0);
    L.bytes = up(L.off[7], 64);
    return L;
}

static inline uint64_t state_fnv(uint64_t h, const void *p, size_t n)
{
    const uint8_t *c = static_cast<const uint8_t *>(p);
    for (size_t k = 0; k < n; k++)
        h = (h ^ c[k]) * 0x100000001b3ULL;
    return h;
}

// The topology as mmc_batch_create was given it (mmc_state_info::topology).
static inline uint64_t state_topology(int64_t n_mol, const int64_t *atype, const double *charge, int64_t n_types,
                               const double *eps, const double *sig)
{
    uint64_t h = 0xcbf29ce484222325ULL;
    h = state_fnv(h, &n_types, sizeof(n_types));
    h = state_fnv(h, atype, sizeof(int64_t) * 3 * n_mol);
    h = state_fnv(h, charge, sizeof(double) * 3 * n_mol);
    h = state_fnv(h, eps, sizeof(double) * n_types * n_types);
    return state_fnv(h, sig, sizeof(double) * n_types * n_types);
}

// The fixed solute as mmc_batch_set_solute was given it (mmc_state_info::solute_hash): FNV-1a over
// n_sites (8 bytes) and the five arrays mol [S + 1][3], charge [S], eps [S][3], sig [S][3].
static inline uint64_t state_solute_hash(int64_t n_sites, const double *mol, const double *charge, const double *eps,
                                         const double *sig)
{
    uint64_t h = 0xcbf29ce484222325ULL;
    h = state_fnv(h, &n_sites, sizeof(n_sites));
    h = state_fnv(h, mol, sizeof(double) * 3 * (n_sites + 1));
    h = state_fnv(h, charge, sizeof(double) * n_sites);
    h = state_fnv(h, eps, sizeof(double) * 3 * n_sites);
    return state_fnv(h, sig, sizeof(double) * 3 * n_sites);
}

#define ST_FLAG_PER_BOX 1u
#define ST_FLAG_TEMPS 2u
#define ST_FLAG_QUAT 4u

#ifdef __HIPCC__
#define ST_BLOCK 256
#define ST_SLAB 128 // molecules of one workgroup: even, so that a slab's part of a section starts on 16 bytes

struct StateArgs {
    int64_t off_com, off_coords, off_S, off_quat, off_end, rec_bytes;
    int r0;                // the chunk's first replica: workgroup (s, y) works on replica r0 + y, record y
    int n_slabs;           // gridDim.x
    int quat;              // the records carry orientations
    int per_box;           // unpack: the fixed-point centres of mass are fractions of the record's own box
    const double *d_box;   // pack: [R] per-replica boxes, or null: `box`
    double box;
    const double *d_temps; // pack: [R] or null (0.0)
    const uint8_t *cur;    // pack: [R] which S buffer of a replica is sumQExpOld
    unsigned long long flags;
};

typedef unsigned long long st_u64x2 __attribute__((ext_vector_type(2)));

// A slab of molecules as [m][12] doubles (atoms x0 y0 z0 .. z2, then the centre of mass), the order of
// the first 96 bytes of a per-molecule record line.
template <bool REC>
__device__ __forceinline__ void state_load_slab(const BatchView &bv, const double *rec, int r, int j0, int nj,
                                                double2 *tile2)
{
    double *tile = reinterpret_cast<double *>(tile2);
    if (REC) {
        const double2 *src = reinterpret_cast<const double2 *>(rec + ((int64_t)r * bv.n_mol + j0) * MMC_RSTRIDE);
        for (int u = threadIdx.x; u < nj * 6; u += ST_BLOCK)
            tile2[u] = src[(u / 6) * (MMC_RSTRIDE / 2) + u % 6];
    } else {
        const int64_t a0 = (int64_t)r * bv.atom_stride + 3 * (int64_t)j0, m0 = (int64_t)r * bv.mol_stride + j0;
        for (int u = threadIdx.x; u < nj * 3; u += ST_BLOCK) {
            double *o = tile + (u / 3) * 12 + 3 * (u % 3);
            o[0] = bv.ax[a0 + u]; o[1] = bv.ay[a0 + u]; o[2] = bv.az[a0 + u];
        }
        for (int u = threadIdx.x; u < nj; u += ST_BLOCK) {
            double *o = tile + u * 12 + 9;
            o[0] = bv.comx[m0 + u]; o[1] = bv.comy[m0 + u]; o[2] = bv.comz[m0 + u];
        }
    }
}

// Records of replicas [a.r0, a.r0 + gridDim.y) to out[y * rec_bytes]: grid (slabs, replicas), a
// workgroup per (replica, slab of ST_SLAB molecules).  Homogeneous systems (REC) read the 128-byte
// record lines, the others the SoA arrays; S(k) and the orientations are 16-byte copies spread over
// the replica's workgroups.  Every byte of a record is written, padding as zero.
template <bool REC>
__global__ __launch_bounds__(ST_BLOCK) void k_state_pack(BatchView bv, const double *rec, StateArgs a, uint8_t *out)
{
    __shared__ double2 tile2[ST_SLAB * 6];
    const double *tile = reinterpret_cast<const double *>(tile2);
    const int s = blockIdx.x, r = a.r0 + blockIdx.y, tid = threadIdx.x;
    uint8_t *o = out + (int64_t)blockIdx.y * a.rec_bytes;
    const int j0 = s * ST_SLAB, nj = min(ST_SLAB, bv.n_mol - j0);
    state_load_slab<REC>(bv, rec, r, j0, nj, tile2);
    __syncthreads();
    { // coords: doubles [9 j0, 9 (j0 + nj)) of the section (an odd count ends in the section's padding)
        double2 *dst = reinterpret_cast<double2 *>(o + a.off_coords) + (int64_t)j0 * 9 / 2;
        const int nd = nj * 9;
        for (int u = tid; u < (nd + 1) / 2; u += ST_BLOCK) {
            const int d0 = 2 * u, d1 = d0 + 1;
            dst[u] = make_double2(tile[(d0 / 9) * 12 + d0 % 9], d1 < nd ? tile[(d1 / 9) * 12 + d1 % 9] : 0.0);
        }
    }
    { // com
        double2 *dst = reinterpret_cast<double2 *>(o + a.off_com) + (int64_t)j0 * 3 / 2;
        const int nd = nj * 3;
        for (int u = tid; u < (nd + 1) / 2; u += ST_BLOCK) {
            const int d0 = 2 * u, d1 = d0 + 1;
            dst[u] = make_double2(tile[(d0 / 3) * 12 + 9 + d0 % 3], d1 < nd ? tile[(d1 / 3) * 12 + 9 + d1 % 3] : 0.0);
        }
    }
    {
        const double2 *src = reinterpret_cast<const double2 *>(s_buf(bv, r, a.cur[r]));
        double2 *dst = reinterpret_cast<double2 *>(o + a.off_S);
        for (int u = s * ST_BLOCK + tid; u < bv.nkvecs; u += a.n_slabs * ST_BLOCK)
            dst[u] = src[u];
    }
    if (a.quat) {
        const double2 *src = reinterpret_cast<const double2 *>(bv.quat + (int64_t)r * 4 * bv.n_mol);
        double2 *dst = reinterpret_cast<double2 *>(o + a.off_quat);
        for (int u = s * ST_BLOCK + tid; u < 2 * bv.n_mol; u += a.n_slabs * ST_BLOCK)
            dst[u] = src[u];
    }
    if (s == 0) {
        if (tid == 0) {
            reinterpret_cast<double2 *>(o)[0] =
                make_double2(a.d_box ? a.d_box[r] : a.box, a.d_temps ? a.d_temps[r] : 0.0);
            st_u64x2 f = { a.flags, 0ULL };
            reinterpret_cast<st_u64x2 *>(o)[1] = f;
        }
        if ((int64_t)tid < (a.rec_bytes - a.off_end) / 16) // (up to three: the record ends on 64 bytes)
            reinterpret_cast<double2 *>(o + a.off_end)[tid] = make_double2(0.0, 0.0);
    }
}

// The inverse: record y of in[] into replica a.r0 + y, every layout the kernels read -- the SoA
// arrays, the record lines and the fixed-point centres of mass (REC; com_quant with the replica's
// own box, as every writer of a centre of mass does), S(k) into BOTH buffers, the orientations.
template <bool REC>
__global__ __launch_bounds__(ST_BLOCK) void k_state_unpack(BatchView bv, double *rec, StateArgs a, const uint8_t *in)
{
    __shared__ double2 tile2[ST_SLAB * 6];
    double *tile = reinterpret_cast<double *>(tile2);
    const int s = blockIdx.x, r = a.r0 + blockIdx.y, tid = threadIdx.x;
    const uint8_t *o = in + (int64_t)blockIdx.y * a.rec_bytes;
    const int j0 = s * ST_SLAB, nj = min(ST_SLAB, bv.n_mol - j0);
    {
        const double2 *src = reinterpret_cast<const double2 *>(o + a.off_coords) + (int64_t)j0 * 9 / 2;
        const int nd = nj * 9;
        for (int u = tid; u < (nd + 1) / 2; u += ST_BLOCK) {
            const int d0 = 2 * u, d1 = d0 + 1;
            const double2 v = src[u];
            tile[(d0 / 9) * 12 + d0 % 9] = v.x;
            if (d1 < nd)
                tile[(d1 / 9) * 12 + d1 % 9] = v.y;
        }
    }
    {
        const double2 *src = reinterpret_cast<const double2 *>(o + a.off_com) + (int64_t)j0 * 3 / 2;
        const int nd = nj * 3;
        for (int u = tid; u < (nd + 1) / 2; u += ST_BLOCK) {
            const int d0 = 2 * u, d1 = d0 + 1;
            const double2 v = src[u];
            tile[(d0 / 3) * 12 + 9 + d0 % 3] = v.x;
            if (d1 < nd)
                tile[(d1 / 3) * 12 + 9 + d1 % 3] = v.y;
        }
    }
    __syncthreads();
    if (REC) { // (words 12..15 of a line are never written by anyone: they stay zero)
        double2 *dst = reinterpret_cast<double2 *>(rec + ((int64_t)r * bv.n_mol + j0) * MMC_RSTRIDE);
        for (int u = tid; u < nj * 6; u += ST_BLOCK)
            dst[(u / 6) * (MMC_RSTRIDE / 2) + u % 6] = tile2[u];
    }
    const int64_t a0 = (int64_t)r * bv.atom_stride + 3 * (int64_t)j0, m0 = (int64_t)r * bv.mol_stride + j0;
    for (int u = tid; u < nj * 3; u += ST_BLOCK) {
        const double *p = tile + (u / 3) * 12 + 3 * (u % 3);
        bv.ax[a0 + u] = p[0]; bv.ay[a0 + u] = p[1]; bv.az[a0 + u] = p[2];
    }
    const double inv_box = 1.0 / (a.per_box ? *reinterpret_cast<const double *>(o) : bv.box);
    for (int u = tid; u < nj; u += ST_BLOCK) {
        const double *p = tile + u * 12 + 9;
        bv.comx[m0 + u] = p[0]; bv.comy[m0 + u] = p[1]; bv.comz[m0 + u] = p[2];
        comq_store(bv, r, j0 + u, 0, p[0], inv_box);
        comq_store(bv, r, j0 + u, 1, p[1], inv_box);
        comq_store(bv, r, j0 + u, 2, p[2], inv_box);
    }
    {
        const double2 *src = reinterpret_cast<const double2 *>(o + a.off_S);
        double2 *d0 = reinterpret_cast<double2 *>(s_buf(bv, r, 0)), *d1 = reinterpret_cast<double2 *>(s_buf(bv, r, 1));
        for (int u = s * ST_BLOCK + tid; u < bv.nkvecs; u += a.n_slabs * ST_BLOCK) {
            const double2 v = src[u];
            d0[u] = v;
            d1[u] = v;
        }
    }
    if (a.quat) {
        const double2 *src = reinterpret_cast<const double2 *>(o + a.off_quat);
        double2 *dst = reinterpret_cast<double2 *>(bv.quat + (int64_t)r * 4 * bv.n_mol);
        for (int u = s * ST_BLOCK + tid; u < 2 * bv.n_mol; u += a.n_slabs * ST_BLOCK)
            dst[u] = src[u];
    }
}
#endif // __HIPCC__
