// mmc_solute.hpp -- k_solute_wave: Widom insertion of a FOREIGN rigid solute of S sites (1 <= S <= 16)
// into every replica, one wavefront per INSERTION on the unit -> wave map of k_widom_wave
// (mmc_widom.hpp).  The arithmetic is stated in include/mmc_hip.h ("Foreign solutes"): the change of
// the reference's potential(..., "ewald") when the solute is appended as molecule N + 1,
//   d_lj    = LJ_poly_dU(N+1)     energy.jl:209-290: COM gate on the solute's reference point c, S x 3
//                                 atom pairs per gated water, eps > 0.001, slack r_cut^2 + 100
//   d_real  = EwaldShort(N+1)     ewalds.jl:892-910 -> :293-376: COM gate, overlap (r^2 < 0.5 and
//                                 q_a q_b < 0) -> 0 and flag bit 0, erfc table of the batch (qq_pair)
//   d_recip = factor sum_k cfac_k (2 Re(conj(S_k) s_k) + |s_k|^2) - factor kappa / sqrt(pi) sum_a q_a^2
// The solute is not molecule 1, so nothing of mmc_wave_unit.inc's three-site body applies; the unit
// here is written for S sites:
//   * the solute's sites and its reference point ([S + 1][3], word t in lane t) are drawn by
//     widom_draw -- the same three Philox slots, so c is bit for bit Widom's COM and the cavity
//     probe of the same (seed, draw0 + j, replica) -- or read from the caller's array, and parked in
//     the wave's LDS; its parameters (offset, charge, eps and sig against the three water slots) sit
//     in LDS once per workgroup;
//   * the reciprocal part: lane t < 3 S makes the phase row of (site t / 3, axis t % 3) by the
//     reference's recurrence (phase_row_moderate), then a lane takes a k-vector (unit_k_loop)
//     against the replica's committed S(k) and loops over the S sites;
//   * the pair part: the 16-bit COM prefilter (com_quant) lists the waters that can pass a gate,
//     a lane takes a listed water, gathers its record, applies the reference's exact fp64 gates and
//     runs a wave-uniform loop over the S sites, whose coordinates and parameters are LDS
//     broadcasts, against its three atoms.  The minimum image is taken per atom pair (vector1D),
//     which is right for a solute of any extent;
//   * every lane keeps its own sums over all the waters it takes; they are reduced once per unit in
//     a fixed order (wave_sum_rows), so an insertion's result does not depend on the grid.
// SMAX: the sites the phase tables have room for.  16: 52.5 KB of LDS per workgroup (the tables are
// 4 x 16 x 3 x 11 complex numbers = 33 KB), three workgroups per compute unit; 4: 27.7 KB;
// 0: a solute whose charges are all zero -- no reciprocal part, no erfc table, S(k) is not read,
// d_real and d_recip are +0.0 -- 6.9 KB.
// k_widom_reduce (mmc_widom.hpp) then forms the weights and the per-replica sums as it stands.
// Nothing the chains own is written.
#pragma once
#include "mmc_widom.hpp"

#define SOL_MAX_SITES 16 // == MMC_SOLUTE_MAX_SITES (include/mmc_hip.h)
#define SOL_PAR 10       // doubles per site of the parameter block: offset (3), charge, eps (3), sig (3)
#define SOL_LIST 512     // neighbour-list slots per wave: emptied when fewer than 256 are free
#define SOL_WORDS (3 * SOL_MAX_SITES + 4) // the solute's words per wave (3 S + 3 used), 16-byte multiple
// waves per SIMD the instantiations are compiled for and their launches are capped at.  (The
// uncharged instantiation fits 8 -- 61 VGPRs, 6.9 KB -- and was measured there: 6 % faster at 4096
// replicas, 12 % slower at 61440, profiles/solute_occ_ab.json; it stays at 4.)
#define SOL_OCC(SMAX) ((SMAX) == 16 ? 3 : 4)

struct SoluteArgs {
    uint64_t seed;        // Philox key
    int64_t draw0;        // counter of insertion j: draw0 + j
    const double *par;    // [S][SOL_PAR] the solute (device memory)
    const double *mol_in; // [R][M][S + 1][3] caller-given solutes (sites, then c), or NULL: generate
    double *mol_out;      // [R][M][S + 1][3] the evaluated solutes, or NULL
    double *terms;        // [R][M][4]: d_lj, d_real, d_recip + self, (k_widom_reduce:) weight
    uint8_t *flags;       // [R][M]
    const uint8_t *scur;  // [R] which S buffer holds the replica's committed S(k)
    int32_t n_insert;     // M
    int32_t n_sites;      // S
    double self_d;        // -factor kappa / sqrt(pi) sum_a q_a^2 (the host's arithmetic)
};

template <int SMAX> struct SoluteShared {
    alignas(16) double qtab[MMC_QQ_TABLE_DOUBLES];
    cplx ptab[WV_WAVES][SMAX][3][MMC_NKTAB]; // phase rows of the solute's sites
    alignas(16) double par[SOL_MAX_SITES][SOL_PAR];
    alignas(16) double mol[WV_WAVES][SOL_WORDS];
    wv_list_t list[WV_WAVES][SOL_LIST];
};
template <> struct SoluteShared<0> {
    alignas(16) double par[SOL_MAX_SITES][SOL_PAR];
    alignas(16) double mol[WV_WAVES][SOL_WORDS];
    wv_list_t list[WV_WAVES][SOL_LIST];
};
static_assert(3 * sizeof(SoluteShared<16>) <= 160 * 1024, "three workgroups per compute unit");

// grid: any number of workgroups of WV_WAVES waves; wave w of workgroup g takes units
// g * WV_WAVES + w, + gridDim.x * WV_WAVES, ... (k_move_eval_wave's map).  Unit u = insertion
// u % M of replica u / M.  The host launches SMAX >= n_sites, or 0 for an uncharged solute.
template <int SMAX>
__global__ __launch_bounds__(WV_WAVES * 64) __attribute__((amdgpu_waves_per_eu(SOL_OCC(SMAX), SOL_OCC(SMAX)))) void k_solute_wave(
    BatchView bv, const double *__restrict__ rec, const double *__restrict__ qq_tab,
    const int32_t *__restrict__ kpack, FastConsts fc, PairParams pp, SoluteArgs sa, int n_units)
{
    constexpr bool QQ = SMAX > 0;
    __shared__ __align__(16) SoluteShared<SMAX> sm;
    const int tid = threadIdx.x, lane0 = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int S = sa.n_sites, nw = 3 * S + 3;
    if constexpr (QQ)
        for (int k = tid; k < MMC_QQ_TABLE_DOUBLES; k += WV_WAVES * 64)
            sm.qtab[k] = qq_tab[k];
    for (int k = tid; k < S * SOL_PAR; k += WV_WAVES * 64)
        (&sm.par[0][0])[k] = sa.par[k];
    __syncthreads(); // the only workgroup barrier
    const int n_mol = bv.n_mol, nkv = bv.nkvecs;
    const double box = bv.box;
    const BoxConsts bc = box_consts(box);
    const double inv_box = 1.0 / box;
    const uint32_t gate_q = com_quant_gate(fmax(pp.lj_gate_sq, pp.qq_gate_sq), box);
    wv_list_t *const list = sm.list[wv];
    double *const mol = sm.mol[wv];
    const int M = sa.n_insert;
    (void)nkv; (void)kpack; (void)fc;

    UNIT_FOR(unit) {
        const int lane = unit_lane(lane0);
        const int r = unit / M, jins = unit - r * M;
        const double *const myrec = rec + (int64_t)r * n_mol * MMC_RSTRIDE;

        // ---- the solute: word t of [S + 1][3] (sites, then c) in lane t ----
        double mw = 0.0;
        if (sa.mol_in) {
            if (lane < nw)
                mw = sa.mol_in[(int64_t)unit * nw + lane];
        } else {
            double com[3], Rm[3][3];
            widom_draw(sa.seed, (uint64_t)(sa.draw0 + jins), (uint32_t)r, box, com, Rm);
            // lane t < 3 S: site t / 3, axis t % 3 = c + R . offset (k_widom_wave's expression)
            const int t = lane < 3 * S ? lane : 0, a = t / 3, d = t - 3 * a;
            const double r0 = d == 0 ? Rm[0][0] : d == 1 ? Rm[1][0] : Rm[2][0];
            const double r1 = d == 0 ? Rm[0][1] : d == 1 ? Rm[1][1] : Rm[2][1];
            const double r2 = d == 0 ? Rm[0][2] : d == 1 ? Rm[1][2] : Rm[2][2];
            const double o0 = sm.par[a][0], o1 = sm.par[a][1], o2 = sm.par[a][2];
            const double c = d == 0 ? com[0] : d == 1 ? com[1] : com[2];
            const double at = c + ((r0 * o0 + r1 * o1) + r2 * o2);
            const int e = lane - 3 * S;
            mw = e < 0 ? at : e == 0 ? com[0] : e == 1 ? com[1] : e == 2 ? com[2] : 0.0;
        }
        if (lane < nw) {
            if (sa.mol_out)
                sa.mol_out[(int64_t)unit * nw + lane] = mw;
            mol[lane] = mw;
        }
        wave_sync();

        // ---- reciprocal part: s_k of the solute against S_k, cfac (|S + s|^2 - |S|^2) ----
        double s_rec = 0.0;
        if constexpr (QQ) {
            if (lane < 3 * S)
                phase_row_moderate(mw, box, sm.ptab[wv][lane / 3][lane % 3]);
            wave_sync();
            const double *So = s_buf(bv, r, sa.scur[r]);
            double a_rec = 0.0;
            unit_k_loop(bv, kpack, So, nkv, lane, [&](double wgt, double2 so, int kx, int ky, int kz) {
                double sr = 0.0, si = 0.0;
                for (int l = 0; l < S; l++) { // wave-uniform
                    const cplx tn = c_mul_fused(c_mul_fused(sm.ptab[wv][l][0][5 + kx], sm.ptab[wv][l][1][ky]),
                                                sm.ptab[wv][l][2][kz]);
                    const double q = sm.par[l][3];
                    sr = fma(q, tn.re, sr);
                    si = fma(q, tn.im, si);
                }
                const double s2 = fma(sr, sr, si * si);
                a_rec = fma(wgt, fma(2.0, fma(so.x, sr, so.y * si), s2), a_rec);
            });
            s_rec = wave_sum_rows(a_rec);
        }

        // ---- pair part ----
        const double cx = mol[3 * S], cy = mol[3 * S + 1], cz = mol[3 * S + 2];
        const uint32_t cqxy = (uint32_t)com_quant(cx, inv_box) | (uint32_t)com_quant(cy, inv_box) << 16;
        const uint32_t cqz = (uint32_t)com_quant(cz, inv_box);
        double a_lj = 0.0, a_q = 0.0;    // this lane's sums over every water it takes
        unsigned long long ovm = 0ULL;   // lanes that saw an overlap

        // neighbours list[0 .. cnt): lane n takes neighbour n0 + n
        auto process = [&](int cnt) {
            wave_sync();
            for (int n0 = 0; n0 < cnt; n0 += 64) {
                const int n = n0 + lane;
                const bool act = n < cnt;
                const int j = act ? list[n] : 0; // idle lanes: molecule 0, gates forced off
                double t[MMC_REC];
                const double2 *src = reinterpret_cast<const double2 *>(myrec + (int64_t)j * MMC_RSTRIDE);
#pragma unroll
                for (int q = 0; q < 6; q++) {
                    const double2 v = src[q];
                    t[2 * q] = v.x;
                    t[2 * q + 1] = v.y;
                }
                // the gates, exactly: COM minimum image on the reference's arithmetic
                // (energy.jl:248-254, ewalds.jl:334-340)
                const double gx = vector1D_abs(cx, t[9], bc), gy = vector1D_abs(cy, t[10], bc),
                             gz = vector1D_abs(cz, t[11], bc);
                const double c2 = gx * gx + gy * gy + gz * gz;
                const bool g = QQ && act && (c2 < pp.qq_gate_sq);
                const bool l = act && (c2 < pp.lj_gate_sq);
                if (!wave_any(g || l))
                    continue;
                for (int a = 0; a < S; a++) { // wave-uniform: the site's words are LDS broadcasts
                    const double *p = sm.par[a];
                    const double ax = mol[3 * a], ay = mol[3 * a + 1], az = mol[3 * a + 2];
#pragma unroll
                    for (int b = 0; b < 3; b++) {
                        const double px = vector1D_abs(ax, t[3 * b], bc), py = vector1D_abs(ay, t[3 * b + 1], bc),
                                     pz = vector1D_abs(az, t[3 * b + 2], bc);
                        const double u = px * px + py * py + pz * pz;
                        if constexpr (QQ) {
                            const double qq = p[3] * fc.q[b];
                            const bool ov = g && (u < pp.ovr) && (qq < 0.0); // ewalds.jl:359
                            ovm |= wave_ballot(ov);
                            double e = 0.0;
                            if (g && !ov && u < pp.qq_slack_sq) // :362
                                e = qq_pair(sm.qtab, u, pp.kappa);
                            a_q = fma(e, qq, a_q); // :365-367
                        }
                        const double eps = p[4 + b];
                        if (l && u < pp.lj_slack_sq && eps > 0.001) { // energy.jl:270
                            const double sg = p[7 + b];
                            const double s2 = sg * sg / u;
                            const double s6 = s2 * s2 * s2;
                            const double s12 = s6 * s6;
                            a_lj += eps * (s12 - s6);
                        }
                    }
                }
            }
            wave_sync();
        };

        // COM scan on the 16-bit box fractions (com_quant: the wrapped difference is the minimum
        // image, gate_q admits every water an exact gate can accept): lane per water, four blocks
        // of 64 in flight, survivors appended in ascending j.  The index is clamped, so nothing
        // past the replica's codes is read.
        {
            const uint16_t *cq = bv.comq + (int64_t)r * 3 * bv.cq_stride;
            const uint32_t *cq_xy = reinterpret_cast<const uint32_t *>(cq);
            const uint16_t *cq_z = cq + 2 * bv.cq_stride;
            int cnt = 0;
            for (int base = 0; base < n_mol; base += 256) {
                uint32_t fxy[4], fz[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int jc = min(base + 64 * q + lane, n_mol - 1);
                    fxy[q] = cq_xy[jc];
                    fz[q] = cq_z[jc];
                }
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int j = base + 64 * q + lane;
                    const bool keep = j < n_mol && com_quant_dist2(fxy[q], fz[q], cqxy, cqz) < gate_q;
                    const unsigned long long m = wave_ballot(keep);
                    if (keep)
                        list[cnt + lanes_below(m)] = (wv_list_t)j;
                    cnt += __popcll(m);
                }
                if (cnt > SOL_LIST - 256) { // no room for another four blocks: empty the list
                    process(cnt);
                    cnt = 0;
                }
            }
            if (cnt)
                process(cnt);
        }

        // ---- the unit's three terms and its overlap flag (unit_store_terms' arithmetic) ----
        const double s_lj = wave_sum_rows(a_lj);
        const double s_q = QQ ? wave_sum_rows(a_q) : 0.0;
        if (lane == 0) {
            const int ov = ovm != 0ULL;
            double *t = sa.terms + (int64_t)unit * 4;
            t[0] = (0.0 + s_lj) * 4;                       // energy.jl:289
            if constexpr (QQ) {
                double d_real = ov ? 0.0 : 0.0 + s_q;      // ewalds.jl:359-360
                d_real *= bv.factor;                       // ewalds.jl:905
                t[1] = d_real;
                t[2] = s_rec * bv.factor + sa.self_d;
            } else {
                t[1] = 0.0;
                t[2] = 0.0;
            }
            sa.flags[unit] = (uint8_t)(ov ? MMC_WIDOM_OVERLAP : 0);
        }
        wave_sync(); // (mol, list and ptab are rewritten by this wave's next unit)
    }
}
