// mmc_widom.hpp -- k_widom_wave: Widom test-particle insertion on the wave-per-unit scheme of
// k_move_eval_wave (mmc_wave.hpp), one wavefront per INSERTION.
//
// The reference has no insertion code; the insertion energy is defined through its own total
// energy (include/mmc_hip.h, mmc_batch_widom): the change of potential(..., "ewald")
// (Ewald/energy.jl:946-1032) when a rigid copy of molecule 1 is appended as molecule N + 1,
//   dU = LJ_poly_dU(N+1)                       energy.jl:209-290
//      + EwaldShort(N+1)                       ewalds.jl:892-910 -> EwaldReal :293-376
//      + factor sum_k cfac_k (2 Re(conj(S_k) s_k) + |s_k|^2)     RecipLong(N+1) - RecipLong(N), :538-604
//      - factor kappa / sqrt(pi) sum_a q_a^2   EwaldSelf(N+1) - EwaldSelf(N), :829-833
// An insertion is the "new state" half of a trial move with no old state, no commit and no
// decision, so the unit is that half of k_move_eval_wave's:
//   * the test molecule (drawn here from the replica's Philox stream, or the caller's for
//     mmc_batch_widom_at) is one lane-distributed register in MoveRec layout, pulled into scalars
//     where it is used;
//   * the reciprocal part: the phase rows of its three atoms (phase_row_moderate, the reference's
//     recurrence), then lane per k over the half-space list against the replica's CURRENT S(k);
//   * the pair part is mmc_wave_unit.inc itself with one state (WV_NS = 1, as the context server
//     evaluates one molecule): 16-bit COM prefilter, exact fp64 gate on the gathered records, lane
//     per neighbour, erfc table, the cold series below r^2 = 0.25, overlap by ewalds.jl:359;
//   * lane 0 combines the sums (mmc_combine_parts' arithmetic for one state) and stores the three
//     terms and the overlap flag of the insertion.
// k_widom_reduce then takes the weights exp(-dU / T) and adds each replica's in insertion order, so
// the sums do not depend on
// the grid, on "wave_wgs" or on how many insertions a persistent wave takes.
// Nothing the chains own is written: coordinates, S(k), flags and step counters are only read.
#pragma once
#include "mmc_unit.hpp"

#ifndef WIDOM_OCC
#define WIDOM_OCC 4 // waves per SIMD k_widom_wave is compiled for: 102 VGPRs, no scratch (at 5 = 96 VGPRs
#endif              // it spilled 5 VGPRs: the test molecule's record and the insertion's bookkeeping)
#define MMC_WIDOM_SLOT 0x50000000u // == MMC_SLOT_WIDOM (include/mmc_hip.h): slots +0, +1, +2 (+3..+5: mmc_solute_pair.hpp)

struct WidomArgs {
    uint64_t seed;       // Philox key
    int64_t draw0;       // counter of insertion j: draw0 + j
    const double *off;   // [9] body offsets of the three atoms from the COM (generated insertions;
                         // device memory: scalar loads where they are used, not 18 SGPRs for the kernel's life)
    const double *mol_in; // [R][M][12] caller-given molecules (atoms, COM), or NULL: generate
    double *mol_out;     // [R][M][12] the evaluated molecules, or NULL
    double *terms;       // [R][M][4]: d_lj, d_real, d_recip + self, (k_widom_reduce:) weight
    uint8_t *flags;      // [R][M]
    const uint8_t *scur; // [R] which S buffer holds the replica's committed S(k)
    int32_t n_insert;    // M
    double self_d;       // -factor kappa / sqrt(pi) sum_a q_a^2 (the host's arithmetic)
};

// Shoemake's uniform unit quaternion from three uniforms, as a rotation matrix
__device__ __forceinline__ void shoemake_matrix(double u1, double u2, double u3, double Rm[3][3])
{
    const double s1 = sqrt(1.0 - u1), s2 = sqrt(u1);
    double sa, ca, sb, cb;
    sincos(MMC_TWOPI * u2, &sa, &ca);
    sincos(MMC_TWOPI * u3, &sb, &cb);
    const double qw = s2 * cb, qx = s1 * sa, qy = s1 * ca, qz = s2 * sb;
    Rm[0][0] = 1.0 - 2.0 * (qy * qy + qz * qz);
    Rm[0][1] = 2.0 * (qx * qy - qw * qz);
    Rm[0][2] = 2.0 * (qx * qz + qw * qy);
    Rm[1][0] = 2.0 * (qx * qy + qw * qz);
    Rm[1][1] = 1.0 - 2.0 * (qx * qx + qz * qz);
    Rm[1][2] = 2.0 * (qy * qz - qw * qx);
    Rm[2][0] = 2.0 * (qx * qz - qw * qy);
    Rm[2][1] = 2.0 * (qy * qz + qw * qx);
    Rm[2][2] = 1.0 - 2.0 * (qx * qx + qy * qy);
}

// The COM, u L per axis (boundaries.jl:16-26: [0, L)), and the orientation, Shoemake's of the next three
// uniforms.  Host mirror: metropolismontecarlo_amd/observables.py widom_molecules.
__device__ __forceinline__ void widom_draw(uint64_t seed, uint64_t ctr, uint32_t replica, double box,
                                           double com[3], double Rm[3][3])
{
    const ChainKey ck{ seed, replica };
    const Uniform2 d0 = mmc_draw(ck, ctr, MMC_WIDOM_SLOT), d1 = mmc_draw(ck, ctr, MMC_WIDOM_SLOT + 1),
                   d2 = mmc_draw(ck, ctr, MMC_WIDOM_SLOT + 2);
    com[0] = d0.a * box;
    com[1] = d0.b * box;
    com[2] = d1.a * box;
    shoemake_matrix(d1.b, d2.a, d2.b, Rm);
}

// grid: any number of workgroups of WV_WAVES waves; wave w of workgroup g takes units
// g * WV_WAVES + w, + gridDim.x * WV_WAVES, ... (k_move_eval_wave's map).  Unit u = insertion
// u % M of replica u / M.  IMG: as k_move_eval_wave's (the host checks the condition with the test
// molecule's own extent).
template <bool IMG>
__global__ __launch_bounds__(WV_WAVES * 64) __attribute__((amdgpu_waves_per_eu(WIDOM_OCC, WIDOM_OCC))) void k_widom_wave(
    BatchView bv, const double *__restrict__ rec, const double *__restrict__ qq_tab,
    const int32_t *__restrict__ kpack, FastConsts fc, PairParams pp, WidomArgs wa, int n_units)
{
    UNIT_PROLOGUE();
    const double *const pvw = sm.pvw[wv]; // (unused: no pending commit)
    const int M = wa.n_insert;

    UNIT_FOR(unit) {
        const int lane = unit_lane(lane0);
        const int r = unit / M, jins = unit - r * M;
        const double *const myrec = rec + (int64_t)r * n_mol * MMC_RSTRIDE;

        // ---- the test molecule: word t of its record (atoms 0..8, COM 9..11) in lane t ----
        double mw = 0.0;
        if (wa.mol_in) {
            if (lane < MMC_REC)
                mw = wa.mol_in[(int64_t)unit * MMC_REC + lane];
        } else {
            double com[3], Rm[3][3];
            widom_draw(wa.seed, (uint64_t)(wa.draw0 + jins), (uint32_t)r, box, com, Rm);
            // lane t < 9: atom t / 3, axis t % 3 = COM + R . offset; lanes 9..11: the COM
            const int t = lane < 9 ? lane : 0, a = t / 3, d = t - 3 * a;
            const double r0 = d == 0 ? Rm[0][0] : d == 1 ? Rm[1][0] : Rm[2][0];
            const double r1 = d == 0 ? Rm[0][1] : d == 1 ? Rm[1][1] : Rm[2][1];
            const double r2 = d == 0 ? Rm[0][2] : d == 1 ? Rm[1][2] : Rm[2][2];
            const double o0 = a == 0 ? wa.off[0] : a == 1 ? wa.off[3] : wa.off[6];
            const double o1 = a == 0 ? wa.off[1] : a == 1 ? wa.off[4] : wa.off[7];
            const double o2 = a == 0 ? wa.off[2] : a == 1 ? wa.off[5] : wa.off[8];
            const double c = d == 0 ? com[0] : d == 1 ? com[1] : com[2];
            const double at = c + ((r0 * o0 + r1 * o1) + r2 * o2);
            mw = lane < 9 ? at : lane == 9 ? com[0] : lane == 10 ? com[1] : lane == 11 ? com[2] : 0.0;
        }
        if (wa.mol_out && lane < MMC_REC)
            wa.mol_out[(int64_t)unit * MMC_REC + lane] = mw;
        const double w = unit_proposal_slot(mw, lane);

        // reciprocal part: s_k of the test molecule against S_k, cfac (|S + s|^2 - |S|^2)
        unit_recip_energy<+1>(sm, wv, bv, kpack, fc, r, wa.scur[r], mw, lane, nkv, box);

        // ================= pair part: mmc_wave_unit.inc, one state =================
        const int i0 = -1, pend = -1, scur = 0;
        const bool do_pairs = true, do_recip = false;
        const int j_begin = 0, j_end = n_mol;
        (void)scur; (void)pvw;
#define WV_NS 1
#define WV_SUBST 0
#define WV_IMG IMG
#define WV_UNIT_NO_STORE
#define WV_CQ_BASE (bv.comq + (int64_t)r * 3 * bv.cq_stride)
#include "mmc_wave_unit.inc"
#undef WV_CQ_BASE
#undef WV_UNIT_NO_STORE
#undef WV_IMG
#undef WV_SUBST
#undef WV_NS
        unit_store_terms(sm, wv, lane, bv.factor, wa.self_d, wa.terms + (int64_t)unit * 4, wa.flags + unit);
    }
}

// One wave per replica: the weights exp(-dU / T), dU = (d_lj + d_real) + d_recip, of blocks of 64
// insertions (lane per insertion; a flagged or non-finite dU weighs 0 and counts), then
// boltz[r] += w_0 + w_1 + ... in insertion order, n_ovl[r] += the flagged ones.  The
// terms of the next block are loaded while this one is added (one replica of 61 440 insertions is
// 960 blocks in a row).
__global__ __launch_bounds__(64) void k_widom_reduce(double *__restrict__ terms, uint8_t *__restrict__ flags,
                                                     int M, double inv_temp, double *boltz, long long *n_ovl)
{
    __shared__ double wsh[64];
    const int r = blockIdx.x, lane = threadIdx.x;
    double *t = terms + (int64_t)r * M * 4;
    uint8_t *f = flags + (int64_t)r * M;
    double acc = boltz[r];
    long long cnt = 0;
    auto load = [&](int i, double &a, double &b, double &c, int &fl) {
        const bool ok = i < M;
        const int k = ok ? i : 0;
        a = t[(int64_t)k * 4]; b = t[(int64_t)k * 4 + 1]; c = t[(int64_t)k * 4 + 2];
        fl = ok ? f[k] : 0;
    };
    double n0, n1, n2;
    int nf;
    load(lane, n0, n1, n2, nf);
    for (int b = 0; b < M; b += 64) {
        const int i = b + lane;
        const int nb = min(64, M - b);
        const double t0 = n0, t1 = n1, t2 = n2;
        int fl = nf;
        load(i + 64, n0, n1, n2, nf);
        double wt = 0.0;
        if (i < M) {
            const double du = (t0 + t1) + t2;
            fl |= isfinite(du) ? 0 : MMC_WIDOM_NONFINITE;
            wt = fl ? 0.0 : exp(-du * inv_temp);
            t[(int64_t)i * 4 + 3] = wt;
            f[i] = (uint8_t)fl;
        }
        cnt += __popcll(wave_ballot(i < M && fl != 0));
        // the block's weights through LDS, read back by every lane alike (broadcast reads that do
        // not depend on the sum, so they run ahead of the chain of additions; the same additions as
        // v_readlane per weight, which cost 2.4 ms per 61 440 insertions in SGPR hazards)
        wsh[lane] = wt;
        wave_sync();
#pragma unroll 8
        for (int q = 0; q < nb; q++)
            acc += wsh[q];
        wave_sync();
    }
    if (lane == 0) {
        boltz[r] = acc;
        n_ovl[r] += cnt;
    }
}
