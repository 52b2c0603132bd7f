// mmc_cand.hpp -- candidate lists of the move kernel's COM scan ("Candidate lists").
//
// k_move_eval_wave tests all n_mol centres of mass of a replica for every trial move, to keep the
// ~1/6 that pass the fixed-point prefilter.  Per replica there is a reference snapshot q0 of the
// codes and, per molecule i, the list cand(i) = { j : dist2(q0_i, q0_j) < t_build } in ascending j
// (i included), t_build the prefilter's threshold for gate + skin.  A step whose chosen molecule's
// list is known to hold every survivor of the prefilter applies the SAME test to the candidates
// only, in the same order: the list the pair loops see is identical, hence every bit after it.
//
// Why the list holds every survivor: the wrapped 16-bit difference per axis is the cyclic distance
// of the codes, so dist = sqrt(dist2) obeys the triangle inequality.  With D_r the largest dist2 of
// any molecule of replica r from its q0 code since the snapshot, a survivor j of a state c of the
// chosen molecule i (dist2(c, cur_j) < gate_q) has
//     dist(q0_i, q0_j) <= dist(q0_i, c) + dist(c, cur_j) + dist(cur_j, q0_j)
//                      <= a + G + sqrt(D_r),    a = dist(q0_i, c), G = ceil(sqrt(gate_q)),
// and is a candidate when that is at most S = floor(sqrt(t_build - 1)).  The step's test is therefore
// a + sqrt(D_r) <= B, B = S - G (cand_budget), made on the squares (cand_within).
//
// D_r lives in device memory.  Every commit of an accepted move either raises it (cand_note_commit:
// the wave kernel's commit block with one part per move, k_settle_rec) or the host marks the replica
// stale, D_r = MMC_CAND_STALE, in stream order (every other writer of BatchView::comq: mmc_batch.inc).
// A stale replica fails the test -- the full scan runs -- until k_cand_refresh has rebuilt it.
#pragma once
#include "mmc_kernels.hpp"

#define MMC_CAND_CAP 256            // indices per molecule (four 64-molecule blocks instead of n_mol / 64)
#define MMC_CAND_STALE 0xffffffffu  // D_r of a replica whose lists describe nothing
#define MMC_CAND_STATS 3            // counters per replica: steps on its lists, steps on the full scan, refreshes

struct CandView {
    uint16_t *idx;            // [R][n_mol][MMC_CAND_CAP] cand(i), ascending; slots past the count hold valid indices
    uint16_t *cnt;            // [R][cq_stride] |cand(i)|, saturated at 0xffff; above MMC_CAND_CAP the list is not used
    uint16_t *q0;             // [R][3 cq_stride] the snapshot, laid out as BatchView::comq
    uint32_t *D;              // [R] D_r, or MMC_CAND_STALE
    unsigned long long *stat; // [R][MMC_CAND_STATS]
    uint32_t budget;          // B for the lists as built (cand_budget)
};

// floor(sqrt(x)) of a 32-bit number, exactly (the double root of an integer below 2^53 is off by less than 1)
__host__ __device__ inline uint32_t cand_isqrt(uint32_t x)
{
    uint32_t s = (uint32_t)sqrt((double)x);
    while ((uint64_t)s * s > x) s--;
    while ((uint64_t)(s + 1) * (s + 1) <= x) s++;
    return s;
}

// B: how far, in code units, dist(q0_i, c) + sqrt(D_r) may go for lists built with t_build and a
// prefilter threshold gate_q (0: never -- the lists are of no use)
__host__ __device__ inline uint32_t cand_budget(uint32_t t_build, uint32_t gate_q)
{
    if (t_build == 0 || gate_q == 0xffffffffu)
        return 0; // (a prefilter that admits everything: the scan keeps every molecule, and so it stays)
    if (t_build == 0xffffffffu)
        return 0xffffu; // every molecule is everyone's candidate, wherever it goes; B^2 stays below MMC_CAND_STALE
    const uint32_t S = cand_isqrt(t_build - 1);
    uint32_t G = cand_isqrt(gate_q);
    if ((uint64_t)G * G < gate_q) G++;
    return S > G ? (S - G < 0xffffu ? S - G : 0xffffu) : 0;
}

// sqrt(a2) + sqrt(d2) <= B, decided on the squares: a2 + d2 + 2 sqrt(a2 d2) <= B^2, the root bounded
// from above by rounding its allowance h DOWN (errs towards the full scan only).  No overflow:
// B <= 65535, so a2, d2 <= B^2 < 2^32 where the products are made and h < 2^31; D_r = MMC_CAND_STALE
// is above every B^2 and always fails.
__host__ __device__ inline bool cand_within(uint32_t a2, uint32_t d2, uint32_t B)
{
    const uint64_t b2 = (uint64_t)B * B, s = (uint64_t)a2 + d2;
    if (s > b2)
        return false;
    const uint64_t h = (b2 - s) >> 1;
    return (uint64_t)a2 * d2 <= h * h;
}

#ifdef __HIPCC__
// One accepted move of molecule m of replica r, new codes (xy, z), has been written to comq: raise
// D_r from d_now.  Every caller is the only writer of replica r at the time; `writer`: the one lane
// that stores (the others of a wave only follow the value).  Returns the new D_r.
__device__ __forceinline__ uint32_t cand_note_commit(const CandView &cv, uint32_t q0xy, uint32_t q0z, int r,
                                                     uint32_t xy, uint32_t z, uint32_t d_now, bool writer)
{
    const uint32_t d2 = com_quant_dist2(xy, z, q0xy, q0z);
    if (d2 > d_now) {
        if (writer)
            cv.D[r] = d2;
        return d2;
    }
    return d_now;
}
// the snapshot's codes of molecule m (x | y << 16, z)
__device__ __forceinline__ uint32_t cand_q0_xy(const CandView &cv, int64_t cq_stride, int r, int m)
{
    return reinterpret_cast<const uint32_t *>(cv.q0 + (int64_t)r * 3 * cq_stride)[m];
}
__device__ __forceinline__ uint32_t cand_q0_z(const CandView &cv, int64_t cq_stride, int r, int m)
{
    return cv.q0[(int64_t)r * 3 * cq_stride + 2 * cq_stride + m];
}

// Rebuild q0, every cand(i) and D_r = 0 of the replicas [r_base, r_base + gridDim.x) whose D_r is above
// d_refresh (MMC_CAND_STALE is above everything); one early exit for the others.  A workgroup of four
// waves per replica, a wave per molecule i in turn, lane per j: the prefilter's own integer test
// against t_build, survivors appended in ascending j (the ballot's order), the first MMC_CAND_CAP kept.
// Runs on the stream of the launches that step these replicas, between two of them.
__global__ __launch_bounds__(256) void k_cand_refresh(BatchView bv, CandView cv, int r_base, uint32_t t_build,
                                                      uint32_t d_refresh)
{
    const int r = r_base + blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    __shared__ uint32_t due; // (one read of D_r for the workgroup: thread 0 rewrites it at the end)
    if (tid == 0)
        due = cv.D[r] > d_refresh ? 1u : 0u;
    __syncthreads();
    if (!due)
        return;
    const int n_mol = bv.n_mol;
    const int64_t cqs = bv.cq_stride;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(bv.comq + (int64_t)r * 3 * cqs);
    uint32_t *dst = reinterpret_cast<uint32_t *>(cv.q0 + (int64_t)r * 3 * cqs);
    for (int64_t k = tid; k < 3 * cqs / 2; k += 256) // (cq_stride is a multiple of 64)
        dst[k] = src[k];
    // (the tests read comq itself, which nothing writes while this kernel runs: no wait for the copy)
    const uint16_t *qz = reinterpret_cast<const uint16_t *>(src) + 2 * cqs;
    for (int i = wv; i < n_mol; i += 4) {
        const uint32_t cxy = src[i], cz = qz[i];
        uint16_t *out = cv.idx + ((int64_t)r * n_mol + i) * MMC_CAND_CAP;
        int cnt = 0;
        for (int j0 = 0; j0 < n_mol; j0 += 64) {
            const int j = j0 + lane;
            const bool keep = j < n_mol && com_quant_dist2(src[j < n_mol ? j : 0], qz[j < n_mol ? j : 0], cxy, cz) < t_build;
            const unsigned long long m = __ballot(keep);
            const int at = cnt + __popcll(m & ((1ULL << lane) - 1ULL));
            if (keep && at < MMC_CAND_CAP)
                out[at] = (uint16_t)j;
            cnt += __popcll(m);
        }
        if (lane == 0)
            cv.cnt[(int64_t)r * cqs + i] = (uint16_t)(cnt > 0xffff ? 0xffff : cnt);
    }
    if (tid == 0) {
        cv.D[r] = 0u;
        cv.stat[(int64_t)r * MMC_CAND_STATS + 2] += 1ULL;
    }
}
#endif
