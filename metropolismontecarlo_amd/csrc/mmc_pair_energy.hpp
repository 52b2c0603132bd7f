// mmc_pair_energy.hpp -- pair-energy distributions of every replica, read-only beside the chains:
//   k_pair_energy_wave   per bin of the slot-0 separation the pair count and the sums of the Coulomb
//                        and the Lennard-Jones energy of the pair of molecules, the histogram of the
//                        pair energy u and per-molecule counts of partners with u < u_hb, every pair
//                        i < j once
//   k_pair_energy_nhb    the per-molecule counts -> the distribution of energetic hydrogen bonds
//
// The separation and its bin are k_orient_corr_wave's bit for bit (row (0,0) of k_rdf_sites_wave:
// st_image of mmc_struct.hpp, tile_bin of mmc_tiles.hpp).  The energy of a pair in range is that of
// the nine atom pairs at the MOLECULE's image: with e_a(m) = vector1D(site 0 of m, atom a of m) and D the imaged site-0 difference,
//     x_ab = (D + e_a(i)) - e_b(j),   r2_ab = (x x + y y) + z z,
//     u_C  = factor sum_ab (q_a q_b) / sqrt(r2_ab),
//     u_LJ = sum_ab (4 eps_ab) (s6 s6 - s6),  s6 = (s2 s2) s2,  s2 = (sig_ab sig_ab) / r2_ab,  eps_ab > 0.001,
// both sums a-major, b-minor (include/mmc_hip.h has the expression tree).  The device takes
// 1 / sqrt(r2) from v_rsq_f64 and two coupled Newton steps (pe_rsqrt: relative error ~2^-51) and
// 1 / r2 as its square, where the header divides, and factors the Coulomb sum as
// sum_a q_a (sum_b q_b / sqrt(r2_ab)) -- twelve products for eighteen, and on records three charges
// in scalar registers for nine products: every term stays within a few ulp of the header's, so u_C
// and u_LJ of a pair below the 2^20 K flag limit are within ~2^-30 K of it (nine terms of at most
// ~2^22 K at 2^-51), against the 2^-21 K the quantum allows.
//
// The tiles of the i < j triangle and a wave's run of them are mmc_tiles.hpp's.  Lane n keeps
// neighbour n of block k across a row of tiles -- site 0 and the two offsets e_1, e_2, nine doubles,
// and in the array instantiation its three charges and atom types.  The chosen side: at the start of a tile the 64 lanes load block c's molecules and form
// their offsets as well, and the walk over the chosen molecules pulls the values out with
// v_readlane -- site 0 for the separation, atom a's offset (and charge and type) at the top of its
// three atom pairs, so that no more than one atom's worth of scalar registers is live -- so
// D + e_a(i) adds a scalar operand and the hot loop has no memory load on records (the array
// instantiation looks eps and sigma up by type: two cached loads per atom pair).  Neither
// instantiation spills a register (profiles/pair_energy_codeobj.txt).
// Only pairs in range (bin <= numbins) compute an energy: the rest costs what orient's row 0 costs.
//
// Counters: per wave in LDS, all 64-bit -- three rows of numbins + 2 slots (pair count, sum Q(u_C),
// sum Q(u_LJ)), the n_ebins + 2 slots of the energy histogram and the count of flagged pairs --
// added to with workgroup-scope LDS atomics, flushed to the global block of the same layout when the
// wave's replica changes (per-replica output), once per workgroup at the end (summed output).
// Q(v) = rint(v 2^20) by the 1.5 2^52 add of mmc_orient.hpp, the offset taken off in the register
// (one integer subtract on the high word): a flagged pair adds to row 0 only, so the rows cannot
// share one offset count as orient's do.  The adds are exact modulo 2^64, so a slot is right
// whenever its true sum fits 63 bits: |sum u| < 2^43 K per slot (include/mmc_hip.h).
//
// Energetic hydrogen bonds: c_m = the unflagged partners of m in range with u < u_hb needs a count
// per molecule across tiles.  The lane that owns neighbour j keeps its count in a register across
// the row of tiles and adds it once to cnt[r][j]; for the chosen side lane ii collects the ballot
// popcounts of chosen molecule ii during the tile and the 64 lanes add them with one vector atomic
// per tile.  cnt is an int32 [R][N] region of the observables' scratch, zeroed per call.
#pragma once
#include "mmc_orient.hpp"
#include "mmc_deletion.hpp"

// MMC_PAIRE_MAX_BINS (include/mmc_hip.h): one wave per workgroup with the largest energy histogram --
// thresholds 8 (numbins + 2) bytes, the LJ constants of the nine atom pairs PE_LJ_BYTES, three 64-bit
// rows 24 (numbins + 2) bytes, 8 (MMC_PAIRE_MAX_EBINS + 2) bytes of energy bins and 8 of the flagged count
#define PE_LJ_BYTES 144             // (4 eps_ab, sig_ab^2) of ab = 0..8
static_assert(32 * (MMC_PAIRE_MAX_BINS + 2) + PE_LJ_BYTES + 8 * (MMC_PAIRE_MAX_EBINS + 2) + 8 <= TILE_LDS_BYTES &&
                  32 * (MMC_PAIRE_MAX_BINS + 3) + PE_LJ_BYTES + 8 * (MMC_PAIRE_MAX_EBINS + 2) + 8 > TILE_LDS_BYTES,
              "MMC_PAIRE_MAX_BINS is what one wave fits");
#define PE_LIMIT 1048576.0          // 2^20 K: a pair with |u_C| or |u_LJ| at or above it is flagged

struct PairEArgs {
    TileArgs ta;
    // records only: every molecule is a copy of the first (FastConsts)
    double q3[3];             // the charges of slots 0..2 (ahead of the rest: the kernel's scalar loads
                              // then fall as they did before TileArgs was split off, and so do its registers)
    unsigned long long *out;  // [wstride] or [R][wstride]: rows [3][numbins + 2], energy bins, flagged; zeroed by the host
    int32_t *cnt;             // [R][n_mol] partners below u_hb, zeroed by the host; NULL: not wanted
    int32_t e_slots;          // n_ebins + 2, or 0: no energy histogram
    int32_t wstride;          // 3 (numbins + 2) + e_slots + 1
    double u_lo, u_hi, scale; // scale = n_ebins / (u_hi - u_lo), the host's fp64 (deletion_slot)
    double u_hb, factor;
    // records only
    const double *lj;                // [9][2] device: (4 eps_ab, sig_ab sig_ab), ab = 3 a + b, copied to LDS
    int32_t lj_mask;                 // bit ab: eps_ab > 0.001 (energy.jl:270)
};

// 1 / sqrt(x): v_rsq_f64 (relative error ~2^-23) and two coupled Newton steps on g ~ sqrt(x),
// h ~ 1 / (2 sqrt(x)).  x = 0 gives NaN (0 inf), a NaN stays one: such a pair is flagged.
__device__ __forceinline__ double pe_rsqrt(double x)
{
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = 0.5 * y;
    double e = fma(-h, g, 0.5);
    g = fma(g, e, g);
    h = fma(h, e, h);
    e = fma(-h, g, 0.5);
    h = fma(h, e, h);
    return h + h;
}

__device__ __forceinline__ long long pe_quant(double v)
{
    return __double_as_longlong(v * MMC_PAIRE_SCALE + OR_MAGIC) - (long long)OR_MAGIC_BITS;
}

// Site 0 and the offsets of molecule m of replica r: o[0..2] = site 0, o[3..5] = e_1, o[6..8] = e_2;
// the array instantiation also gives the three charges and atom types.
template <bool REC>
__device__ __forceinline__ void pe_molecule(const BatchView &bv, const double *__restrict__ rec, int r, int m,
                                            const BoxConsts &bc, double *o, double *q, int *ty)
{
    double t[9];
    load_sites9<REC>(bv, rec, r, m, t);
    if constexpr (!REC) {
        const int f0 = bv.first0[m];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            q[a] = bv.charge[f0 + a];
            ty[a] = bv.atype[f0 + a];
        }
    }
#pragma unroll
    for (int d = 0; d < 3; d++) {
        o[d] = t[d];
        o[3 + d] = vector1D(t[d], t[3 + d], bc);
        o[6 + d] = vector1D(t[d], t[6 + d], bc);
    }
}

// REC: molecules are the 128-byte records of homogeneous batches, charges and LJ constants launch
// constants; else the SoA arrays with per-atom charges and types (three-atom molecules only).
// grid and tiles: mmc_tiles.hpp.
template <bool REC>
__global__ __launch_bounds__(TILE_WAVES * 64) void k_pair_energy_wave(BatchView bv, const double *__restrict__ rec,
                                                                    PairEArgs pa)
{
    extern __shared__ __align__(16) unsigned char pe_lds[];
    const TileArgs &ta = pa.ta;
    const int nb = ta.numbins, rs = nb + 2; // row stride: bins 0 .. numbins, then the slot beyond r_max
    const int ws = pa.wstride, e_slots = pa.e_slots;
    const int tid = threadIdx.x, lane0 = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nw = (int)(blockDim.x >> 6);
    double *const thr = reinterpret_cast<double *>(pe_lds);                                      // [rs]
    const double *const ljc = reinterpret_cast<const double *>(pe_lds + 8 * rs);                 // [9][2]
    unsigned long long *const hall = reinterpret_cast<unsigned long long *>(pe_lds + 8 * rs + PE_LJ_BYTES); // [nw][ws]
    unsigned long long *const hw = hall + wv * ws;
    unsigned long long *const uh = hw + 3 * rs;          // [e_slots] energy bins
    unsigned long long *const fl = hw + 3 * rs + e_slots; // flagged pairs
    if (REC && tid < 18)
        reinterpret_cast<double *>(pe_lds + 8 * rs)[tid] = pa.lj[tid];
    tile_prologue(thr, ta.thr, rs, hall, nw * ws);

    const int n_mol = bv.n_mol, n_types = bv.n_types;
    const float inv_dr = ta.inv_dr, e_max = (float)(nb + 1);
    const bool want_hb = pa.cnt != nullptr;
    const double u_hb = pa.u_hb, factor = pa.factor;

    // counters src[n_src][ws] summed and added to dst[ws] (integers: any order gives the same bits)
    auto flush = [&](unsigned long long *dst, unsigned long long *src, int n_src, int first, int step, bool clear) {
        for (int q = first; q < ws; q += step) {
            unsigned long long v = 0ull;
            for (int w = 0; w < n_src; w++)
                v += src[w * ws + q];
            if (v != 0ull)
                atomicAdd(&dst[q], v);
            if (clear)
                src[q] = 0ull;
        }
    };
    auto flush_wave = [&](unsigned long long *dst) {
        wave_sync();
        flush(dst, hw, 1, lane0, 64, true);
        wave_sync();
    };

    TileCursor tc(ta, gridDim.x, blockIdx.x, nw, wv);
    if (tc.more()) {
        int r_hist = tc.r;
        double t[9];  // neighbour j: site 0, e_1, e_2
        double qj[3]; // ... and, array instantiation, its charges and types
        int tj[3], tjn[3] = { 0, 0, 0 };
        int cj = 0;          // neighbour j's partners below u_hb in this row of tiles
        int64_t cj_at = 0;   // ... and where they go: r n_mol + j
        BoxConsts bc = box_consts(bv.box);
        for (; tc.more(); tc.next()) {
            const int r = tc.r;
            // `lane` is made opaque once per unit (mmc_wave.hpp): lane-derived values are not hoisted
            // out of the persistent loop and held for the kernel's life
            int lane = lane0;
            asm volatile("" : "+v"(lane));
            if (ta.per_replica && r != r_hist) {
                flush_wave(pa.out + (int64_t)r_hist * ws);
                r_hist = r;
            }
            const int j = 64 * tc.k + lane;
            if (tc.fresh) { // neighbour j of replica r (a lane beyond the last molecule loads the last)
                if (want_hb && cj != 0)
                    atomicAdd(&pa.cnt[cj_at], cj);
                cj = 0;
                cj_at = (int64_t)r * n_mol + min(j, n_mol - 1);
                bc = box_consts(ta.box_r ? ta.box_r[r] : bv.box);
                pe_molecule<REC>(bv, rec, r, min(j, n_mol - 1), bc, t, qj, tj);
                if constexpr (!REC) {
#pragma unroll
                    for (int a = 0; a < 3; a++)
                        tjn[a] = tj[a] * n_types; // the column of the eps / sig tables
                }
                tc.fresh = false;
            }
            const double half = bc.half, neg_box = bc.neg;
            // the chosen molecules of block c: lane n holds molecule 64 c + n's values, the walk below
            // reads them as wave-uniform values
            const int i_lo = 64 * tc.c, n_i = min(64, n_mol - i_lo);
            double cs[9], cq[3];
            int cty[3];
            pe_molecule<REC>(bv, rec, r, min(i_lo + lane, n_mol - 1), bc, cs, cq, cty);
            int ci = 0; // chosen molecule i_lo + lane's partners below u_hb in this tile
            for (int ii = 0; ii < n_i; ii++) {
                const int i = i_lo + ii;
                const double sx = lane_f64(cs[0], ii), sy = lane_f64(cs[1], ii), sz = lane_f64(cs[2], ii);
                const double xx = st_image(sx - t[0], half, neg_box);
                const double yy = st_image(sy - t[1], half, neg_box);
                const double zz = st_image(sz - t[2], half, neg_box);
                const double r2 = (xx * xx + yy * yy) + zz * zz;
                const int b = tile_bin(thr, r2, inv_dr, e_max);
                const bool pair = j > i && j < n_mol;
                if (pair)
                    __hip_atomic_fetch_add(&hw[b], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                bool hb = false;
                if (pair && b <= nb) {
                    double sc = 0.0, ulj = 0.0;
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        // P = D + e_a(i) (e_0 = 0); atom a's values are read out of block c's lanes here,
                        // not ahead of the nine pairs: three atoms' worth of scalar registers would spill
                        double px = xx, py = yy, pz = zz;
                        if (a) {
                            px = xx + lane_f64(cs[3 * a], ii);
                            py = yy + lane_f64(cs[3 * a + 1], ii);
                            pz = zz + lane_f64(cs[3 * a + 2], ii);
                        }
                        double qia = 0.0;
                        int tia = 0;
                        if constexpr (!REC) {
                            qia = lane_f64(cq[a], ii);
                            tia = __builtin_amdgcn_readlane(cty[a], ii);
                        }
                        double sa = 0.0; // sum_b q_b / sqrt(r2_ab)
#pragma unroll
                        for (int bq = 0; bq < 3; bq++) {
                            const int ab = 3 * a + bq;
                            const double x = bq ? px - t[3 * bq] : px, y = bq ? py - t[3 * bq + 1] : py,
                                         z = bq ? pz - t[3 * bq + 2] : pz;
                            const double r2ab = (x * x + y * y) + z * z;
                            const double ir = pe_rsqrt(r2ab);
                            const double tb = (REC ? pa.q3[bq] : qj[bq]) * ir;
                            sa = bq ? sa + tb : tb;
                            if constexpr (REC) {
                                if ((pa.lj_mask >> ab) & 1) { // (wave-uniform; the constants one LDS read)
                                    const double s2 = ljc[2 * ab + 1] * (ir * ir), s6 = (s2 * s2) * s2;
                                    ulj += ljc[2 * ab] * (s6 * s6 - s6);
                                }
                            } else {
                                const int idx = tia + tjn[bq];
                                const double ep = bv.eps[idx], sg = bv.sig[idx];
                                const double s2 = (sg * sg) * (ir * ir), s6 = (s2 * s2) * s2;
                                ulj += (ep > 0.001) ? (4.0 * ep) * (s6 * s6 - s6) : 0.0;
                            }
                        }
                        const double ta = (REC ? pa.q3[a] : qia) * sa;
                        sc = a ? sc + ta : ta;
                    }
                    const double uc = factor * sc;
                    if (fabs(uc) < PE_LIMIT && fabs(ulj) < PE_LIMIT) { // (false for a NaN)
                        __hip_atomic_fetch_add(&hw[rs + b], (unsigned long long)pe_quant(uc), __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_WORKGROUP);
                        __hip_atomic_fetch_add(&hw[2 * rs + b], (unsigned long long)pe_quant(ulj), __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_WORKGROUP);
                        const double u = uc + ulj;
                        if (e_slots)
                            __hip_atomic_fetch_add(&uh[deletion_slot(u, pa.u_lo, pa.u_hi, pa.scale, e_slots - 2)], 1ull,
                                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        hb = u < u_hb;
                    } else {
                        __hip_atomic_fetch_add(fl, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
                if (want_hb) {
                    const int n = __popcll(__ballot(hb));
                    cj += hb ? 1 : 0;
                    ci += (lane == ii) ? n : 0;
                }
            }
            if (want_hb && ci != 0) // (ci != 0 only in lanes below n_i)
                atomicAdd(&pa.cnt[(int64_t)r * n_mol + i_lo + lane], ci);
        }
        if (want_hb && cj != 0)
            atomicAdd(&pa.cnt[cj_at], cj);
        if (ta.per_replica)
            flush_wave(pa.out + (int64_t)r_hist * ws);
    }
    if (!ta.per_replica) { // once per workgroup: the waves' counters added up, then added to the total
        __syncthreads();
        flush(pa.out, hall, nw, tid, (int)blockDim.x, false);
    }
}

// cnt[R][n_mol] -> nhb[MMC_PAIRE_NHB] (summed) or [R][MMC_PAIRE_NHB]: the number of molecules with
// k partners below u_hb, the last slot for MMC_PAIRE_NHB - 1 or more.  Workgroup g takes the replicas
// g, g + gridDim.x, ...; a replica belongs to one workgroup, which stores its row (per replica) or
// keeps adding and adds its nine sums to the total at the end (summed; nhb zeroed by the host).
__global__ __launch_bounds__(256) void k_pair_energy_nhb(const int32_t *__restrict__ cnt, int n_mol, int R,
                                                         int per_replica, unsigned long long *nhb)
{
    __shared__ unsigned int h[MMC_PAIRE_NHB];
    const int tid = threadIdx.x;
    if (tid < MMC_PAIRE_NHB)
        h[tid] = 0u;
    __syncthreads();
    for (int r = blockIdx.x; r < R; r += (int)gridDim.x) {
        const int32_t *c = cnt + (int64_t)r * n_mol;
        for (int m = tid; m < n_mol; m += 256)
            atomicAdd(&h[min(c[m], MMC_PAIRE_NHB - 1)], 1u);
        if (per_replica) {
            __syncthreads();
            if (tid < MMC_PAIRE_NHB) {
                nhb[(int64_t)r * MMC_PAIRE_NHB + tid] = h[tid];
                h[tid] = 0u;
            }
            __syncthreads();
        }
    }
    if (!per_replica) {
        __syncthreads();
        if (tid < MMC_PAIRE_NHB && h[tid] != 0u)
            atomicAdd(&nhb[tid], (unsigned long long)h[tid]);
    }
}
