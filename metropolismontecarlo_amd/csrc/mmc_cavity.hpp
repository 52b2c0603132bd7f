// mmc_cavity.hpp -- k_cavity_lane: occupancy statistics p_n(R) and the nearest site of probe points
// in every replica, read-only beside the chains.  The arithmetic is stated in include/mmc_hip.h
// ("Cavities and occupancy") and restated in numpy by tests/cavity_ref.py.
//
// The scheme is mmc_nbr.hpp's with a block of 64 probes as the unit and a LANE per probe -- in a copy of
// this kernel's own (site read, staging, run walk): on Sites, stage_sites and RunCursor its walk over
// the sites compiled to code that ran 1.7 % slower (profiles/nbr_scaffold_bench.json).  A
// persistent workgroup takes a contiguous run of the R ceil(n_probe / 64) blocks; for every replica
// its run touches it copies the replica's site positions into LDS once (24 bytes per molecule, SoA),
// and its waves then take the run's blocks of that replica in turn.  The only workgroup barriers are
// the two around that copy.  Where the positions do not fit beside the counters (STAGE = false) the
// lanes read them from the 128-byte records or the SoA arrays instead.
//
// One block, one wave:
//   point    lane l holds probe 64 block + l: drawn from the replica's Philox stream (bit for bit the
//            COM of widom_draw, mmc_widom.hpp) or the caller's for mmc_batch_cavity_at.
//   walk     every lane walks all N sites in index order.  All lanes read the same address: an LDS
//            broadcast.  r^2 through vector1D_abs (the same bits as the signed image squared); the
//            lane keeps (r^2, j) of its nearest site -- a later site replaces an earlier one only when
//            strictly nearer, so ties stay with the lower index, and for r^2 >= +0 the order of the
//            doubles is the order of their bit patterns -- and, for each radius, the number of sites
//            with r^2 < R_k^2.  The eight compares are skipped for a site that no lane of the wave
//            has inside the largest radius (wave-uniform).  No reduction inside the walk.
//   bins     per probe and radius one LDS atomic on the wave's 32-bit counters; the nearest-site bin
//            is the largest m with e2(m) <= r^2, e2(m) = (m dr)(m dr): two correctly rounded fp64
//            products, the same bits the host forms, found from a square-root guess by stepping
//            down and up against e2 itself -- the square root decides nothing.
// Counters: 32-bit, private to the wave in LDS (K (n_cap + 1) occupancy bins, nn_bins + 1 of the
// nearest site), added to the 64-bit global ones whenever the wave leaves a replica, where the lanes'
// 64-bit moment sums are reduced and added too -- integer adds, any order.
#pragma once
#include "mmc_nbr.hpp"
#include "mmc_propose.hpp"

#define CV_MAX_RADII 8                // == MMC_CAVITY_MAX_RADII (include/mmc_hip.h)
#define CV_SLOT 0x50000000u           // == MMC_SLOT_CAVITY == MMC_SLOT_WIDOM: slots +0 and +1

struct CavityArgs {
    const double *box_r;              // [R] per-replica boxes, or NULL: bv.box
    const double *points_in;          // [R][n_probe][3] caller-given points, or NULL: generate
    double *points_out;               // [R][n_probe][3] or NULL
    unsigned long long *occ_hist;     // [K][n_cap + 1] or [R][K][n_cap + 1], zeroed by the host; NULL: not counted
    unsigned long long *occ_mom;      // [K][2] or [R][K][2], zeroed by the host; NULL: not summed
    unsigned long long *nn_hist;      // [nn_bins + 1] or [R][nn_bins + 1], zeroed by the host; NULL: no bins
    int32_t *count;                   // [R][n_probe][K] or NULL
    double *nn_r2;                    // [R][n_probe] or NULL
    int32_t *nn_idx;                  // [R][n_probe] or NULL
    double rad2[CV_MAX_RADII];        // radii[k] radii[k]; 0 (no r^2 is below it) for k >= K
    double rmax2;                     // rad2[K - 1]
    double dr;                        // nn_max / nn_bins (host fp64)
    uint64_t seed;                    // Philox key
    int64_t draw0;                    // counter of probe j: draw0 + j
    int32_t n_probe, n_radii, n_cap, nn_bins;
    int32_t site;                     // atom slot 0..2, or -1: the stored centre of mass
    int32_t per_replica;
    int32_t R;
};

__device__ __forceinline__ unsigned long long cv_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int m = 32; m > 0; m >>= 1)
        v += wave_shfl_xor_u64(v, m);
    return v; // in every lane
}

// REC: molecules are the 128-byte records of homogeneous batches (atoms in words 0..8, the COM in
// 9..11); else the SoA arrays, slot a of molecule j at first0[j] + a and the COM in comx/comy/comz.
// STAGE: the replica's site positions are copied to LDS.
// grid: any number of workgroups of blockDim.x / 64 waves; workgroup g of G takes the probe blocks
// [R B g / G, R B (g + 1) / G) of the replica-major order, B = ceil(n_probe / 64).
// dynamic LDS: [nw][K (n_cap + 1) + nn_bins + 1] counters (without occ_hist no occupancy bins, without
// nn_hist none of the nearest site), rounded up to 16 bytes, then (STAGE) 3 N doubles.
template <bool REC, bool STAGE>
__global__ __launch_bounds__(NBR_WAVES * 64) void k_cavity_lane(BatchView bv, const double *__restrict__ rec,
                                                               CavityArgs ca)
{
    extern __shared__ __align__(16) unsigned char cv_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nw = (int)(blockDim.x >> 6);
    const int n_mol = bv.n_mol, K = ca.n_radii, cap = ca.n_cap;
    const bool bins = ca.nn_hist != nullptr;
    const int nb = bins ? ca.nn_bins : 0;
    const int n_occ = ca.occ_hist ? K * (cap + 1) : 0, hs = n_occ + (bins ? nb + 1 : 0);
    unsigned *const hw = reinterpret_cast<unsigned *>(cv_lds) + wv * hs;     // [K][cap + 1] then [nb + 1]
    double *const pos = reinterpret_cast<double *>(cv_lds + ((4 * (size_t)nw * hs + 15) & ~(size_t)15));
    for (int q = lane; q < hs; q += 64)
        hw[q] = 0u;
    wave_sync();

    const int B = (ca.n_probe + 63) >> 6;
    const int64_t M = (int64_t)ca.R * B;
    const int64_t m0 = M * blockIdx.x / gridDim.x, m1 = M * (blockIdx.x + 1) / gridDim.x;

    // the site of molecule j (j < n_mol) of replica r, from device memory
    auto fetch = [&](int r, int j, double &x, double &y, double &z) {
        if constexpr (REC) {
            const double *p = rec + ((int64_t)r * n_mol + j) * MMC_RSTRIDE + (ca.site < 0 ? 9 : 3 * ca.site);
            x = p[0]; y = p[1]; z = p[2];
        } else if (ca.site < 0) {
            const int64_t c0 = (int64_t)r * bv.mol_stride + j;
            x = bv.comx[c0]; y = bv.comy[c0]; z = bv.comz[c0];
        } else {
            const int64_t a0 = (int64_t)r * bv.atom_stride + bv.first0[j] + ca.site;
            x = bv.ax[a0]; y = bv.ay[a0]; z = bv.az[a0];
        }
    };

    for (int64_t s0 = m0; s0 < m1;) { // the run's blocks of one replica: [b_lo, b_hi) of replica r
        const int r = (int)(s0 / B);
        const int b_lo = (int)(s0 - (int64_t)r * B);
        const int b_hi = (int)min((int64_t)B, (int64_t)b_lo + (m1 - s0));
        s0 += b_hi - b_lo;
        if constexpr (STAGE) {
            __syncthreads(); // every wave has left the previous replica's positions
            for (int j = tid; j < n_mol; j += (int)blockDim.x) {
                double x, y, z;
                fetch(r, j, x, y, z);
                pos[j] = x; pos[n_mol + j] = y; pos[2 * n_mol + j] = z;
            }
            __syncthreads();
        }
        const double box = ca.box_r ? ca.box_r[r] : bv.box;
        const BoxConsts bc = box_consts(box);
        unsigned long long mom1[CV_MAX_RADII], mom2[CV_MAX_RADII]; // this lane's sums of n_k and n_k^2
#pragma unroll
        for (int k = 0; k < CV_MAX_RADII; k++)
            mom1[k] = mom2[k] = 0ULL;

        for (int pb = b_lo + wv; pb < b_hi; pb += nw) {
            const int jp = pb * 64 + lane;
            const bool valid = jp < ca.n_probe;
            const int64_t g = (int64_t)r * ca.n_probe + (valid ? jp : 0);
            double px, py, pz;
            if (ca.points_in) {
                px = ca.points_in[3 * g]; py = ca.points_in[3 * g + 1]; pz = ca.points_in[3 * g + 2];
            } else {
                const ChainKey ck{ ca.seed, (uint32_t)r };
                const uint64_t ctr = (uint64_t)(ca.draw0 + jp);
                const Uniform2 d0 = mmc_draw(ck, ctr, CV_SLOT), d1 = mmc_draw(ck, ctr, CV_SLOT + 1);
                px = d0.a * box; py = d0.b * box; pz = d1.a * box;
            }
            if (ca.points_out && valid) {
                ca.points_out[3 * g] = px; ca.points_out[3 * g + 1] = py; ca.points_out[3 * g + 2] = pz;
            }

            int cnt[CV_MAX_RADII];
#pragma unroll
            for (int k = 0; k < CV_MAX_RADII; k++)
                cnt[k] = 0;
            double best = __longlong_as_double(0x7ff0000000000000LL); // +inf: the first site replaces it
            int best_j = 0;
            for (int j = 0; j < n_mol; j++) {
                double x, y, z;
                if constexpr (STAGE) {
                    x = pos[j]; y = pos[n_mol + j]; z = pos[2 * n_mol + j];
                } else {
                    fetch(r, j, x, y, z);
                }
                const double dx = vector1D_abs(px, x, bc), dy = vector1D_abs(py, y, bc), dz = vector1D_abs(pz, z, bc);
                const double r2 = (dx * dx + dy * dy) + dz * dz;
                const bool nearer = r2 < best;
                best = nearer ? r2 : best;
                best_j = nearer ? j : best_j;
                if (wave_any(r2 < ca.rmax2)) { // wave-uniform
#pragma unroll
                    for (int k = 0; k < CV_MAX_RADII; k++)
                        cnt[k] += r2 < ca.rad2[k] ? 1 : 0;
                }
            }

            if (valid) {
#pragma unroll
                for (int k = 0; k < CV_MAX_RADII; k++) {
                    if (k < K) {
                        if (n_occ)
                            atomicAdd(&hw[k * (cap + 1) + min(cnt[k], cap)], 1u);
                        mom1[k] += (unsigned long long)cnt[k];
                        mom2[k] += (unsigned long long)cnt[k] * (unsigned long long)cnt[k];
                        if (ca.count)
                            ca.count[g * K + k] = cnt[k];
                    }
                }
                if (bins) {
                    // the largest m in 0..nb with (m dr)(m dr) <= best: e2 is monotone in m
                    auto e2 = [&](int m) { const double e = (double)m * ca.dr; return e * e; };
                    const double gs = fmin(sqrt(best) / ca.dr, (double)nb);
                    int m = gs >= 0.0 ? (int)gs : 0; // (a NaN guess: from 0)
                    while (m > 0 && e2(m) > best)
                        m--;
                    while (m < nb && e2(m + 1) <= best)
                        m++;
                    atomicAdd(&hw[n_occ + m], 1u);
                }
                if (ca.nn_r2)
                    ca.nn_r2[g] = best;
                if (ca.nn_idx)
                    ca.nn_idx[g] = best_j;
            }
        }

        // this wave's counters and moment sums added to the replica's (or the summed) ones and cleared
        wave_sync();
        const int64_t ro = ca.per_replica ? r : 0;
        for (int q = lane; q < hs; q += 64) {
            const unsigned v = hw[q];
            if (v != 0u) {
                unsigned long long *dst = q < n_occ ? ca.occ_hist + ro * n_occ + q
                                                    : ca.nn_hist + ro * (nb + 1) + (q - n_occ);
                atomicAdd(dst, (unsigned long long)v);
                hw[q] = 0u;
            }
        }
#pragma unroll
        for (int k = 0; k < CV_MAX_RADII; k++) {
            if (k < K && ca.occ_mom) { // wave-uniform
                const unsigned long long s1 = cv_wave_sum(mom1[k]), s2 = cv_wave_sum(mom2[k]);
                if (lane == 0 && s1 != 0ULL) {
                    atomicAdd(ca.occ_mom + (ro * K + k) * 2, s1);
                    atomicAdd(ca.occ_mom + (ro * K + k) * 2 + 1, s2);
                }
            }
        }
        wave_sync();
    }
}
