// mmc_solute_pair.hpp -- k_solute_pair_wave: Widom insertion of a PAIR of foreign rigid solutes, A of
// S_A sites and B of S_B sites (S_A + S_B <= 16), B at K separations d_k from A along one random ray:
// the numerator of the potential distribution theorem's g_AB(d) at infinite dilution.  One wavefront
// per INSERTION on the unit -> wave map of k_solute_wave (mmc_solute.hpp); the unit evaluates A and
// all K placements of B.  The arithmetic is stated in include/mmc_hip.h ("Solute pairs"): per
// placement the three terms of k_solute_wave (LJ_poly_dU, EwaldShort, RecipLong + EwaldSelf of the
// solute appended as molecule N + 1), and per separation the A-B interaction x as the reference
// would compute it between molecules N + 1 and N + 2.
//   * A's sites and reference point are k_solute_wave's, word for word (widom_draw, slots +0..+2);
//     B's frame -- the rotated offsets R_B off_b and the ray's direction -- comes from slots +3..+5
//     and is parked in the wave's LDS behind A's words; B's words at separation k are made from it
//     where they are needed (or read from the caller's array);
//   * the reciprocal part: A's phase rows once per unit, B's once per separation
//     (phase_row_moderate), then ONE pass of unit_k_loop per separation gives s^A_k and s^B_k and
//     from them B's single term, the cross term 2 Re(conj(s^A) s^B) and (at the first separation)
//     A's single term;
//   * the pair part runs over the K + 1 placements (A, B_0, B_1, ...) in TILES of PAIR_TILE: one
//     COM scan per tile lists the waters that can pass a gate of ANY of the tile's placements, a
//     lane gathers a listed water's record ONCE and evaluates every placement of the tile against
//     it -- each under the reference's exact fp64 COM gates -- with the tile's accumulators in
//     registers.  The words of the tile's placements sit in the LDS the phase rows used (the
//     reciprocal part is over by then);
//   * every lane's sums are reduced once per placement in a fixed order (wave_sum_rows);
//   * the A-B term of a separation: a lane per site pair (S_A S_B <= 64), the COM gate on
//     vector1D(c_A, c_B), the per-pair image, then wave_sum_rows.
// SMAX = 16: phase tables for 16 sites (A's and the current B's), the LDS of SoluteShared<16> plus
// 80 bytes; SMAX = 0: both solutes uncharged -- no tables, no k loop, S(k) not read, every real and
// recip entry +0.0.  k_pair_reduce forms the weights and the [R] and [R][K] sums in insertion order.
// Nothing the chains own is written.
#pragma once
#include "mmc_solute.hpp"

#define PAIR_MAX_SEP 32                  // == MMC_PAIR_MAX_SEP (include/mmc_hip.h)
#define PAIR_TILE 4                      // placements that share a COM scan and a gather
#define PAIR_STRIDE (3 * SOL_MAX_SITES)  // words of a placement's slot in the tile: 3 S + 3 <= 48 (S <= 15)
#define PAIR_WORDS (3 * SOL_MAX_SITES + 8) // A's words, then B's frame: 3 (S_A + S_B) + 6 <= 54
#define PAIR_OVERLAP_AB 4                // flag bit 2: an A-B site pair overlaps
#define PAIR_NONFINITE_AB 8              // flag bit 3: dU_AB is NaN or +-inf

struct SolutePairArgs {
    uint64_t seed;          // Philox key
    int64_t draw0;          // counter of insertion j: draw0 + j
    const double *par;      // [S_A + S_B][SOL_PAR]: A's sites, then B's (device memory)
    const double *xpar;     // [S_A][S_B][3]: eps_ab, sig_ab, q_a q_b
    const double *dsep;     // [K] separations (generated placements)
    const double *mol_a_in; // [R][M][S_A + 1][3] caller-given A (sites, then c), or NULL: generate
    const double *mol_b_in; // [R][M][K][S_B + 1][3] caller-given B, with mol_a_in
    double *mol_a_out;      // [R][M][S_A + 1][3], or NULL
    double *mol_b_out;      // [R][M][K][S_B + 1][3], or NULL
    double *terms;          // [R][M][1 + 2 K][3]: A, B_0 .. B_K-1, x_0 .. x_K-1, each (lj, real, recip)
    uint8_t *flags;         // [R][M][1 + K]
    const uint8_t *scur;    // [R] which S buffer holds the replica's committed S(k)
    int32_t n_insert;       // M
    int32_t n_a, n_b;       // S_A, S_B
    int32_t n_sep;          // K
    double self_a, self_b;  // -factor kappa / sqrt(pi) sum q^2 of each solute (the host's arithmetic)
};

template <int SMAX> struct PairShared {
    alignas(16) double qtab[MMC_QQ_TABLE_DOUBLES];
    // the reciprocal part's phase rows (A's sites, then the current B's); in the pair part the head of
    // EACH WAVE'S OWN rows holds its tile (pair_tile)
    alignas(16) cplx ptab[WV_WAVES][SMAX][3][MMC_NKTAB];
    alignas(16) double par[SOL_MAX_SITES][SOL_PAR];
    alignas(16) double mol[WV_WAVES][PAIR_WORDS];
    wv_list_t list[WV_WAVES][SOL_LIST];
};
template <> struct PairShared<0> {
    alignas(16) double tile[WV_WAVES][PAIR_TILE * PAIR_STRIDE];
    alignas(16) double par[SOL_MAX_SITES][SOL_PAR];
    alignas(16) double mol[WV_WAVES][PAIR_WORDS];
    wv_list_t list[WV_WAVES][SOL_LIST];
};
static_assert(3 * sizeof(PairShared<16>) <= 160 * 1024, "three workgroups per compute unit");
static_assert(sizeof(double) * PAIR_TILE * PAIR_STRIDE <= sizeof(cplx) * 16 * 3 * MMC_NKTAB, "the tile fits the phase rows");

template <int SMAX> __device__ __forceinline__ double *pair_tile(PairShared<SMAX> &sm, int wv)
{
    if constexpr (SMAX > 0)
        return reinterpret_cast<double *>(&sm.ptab[wv][0][0][0]);
    else
        return sm.tile[wv];
}

// B's frame from slots MMC_SLOT_WIDOM + 3, 4, 5: the ray's direction nh = (s cos phi, s sin phi, z),
// z = 1 - 2 u, s = sqrt(1 - z^2), phi = 2 pi v of slot +3; Shoemake's rotation of (u1, u2) = slot +4
// and u3 = the first uniform of slot +5 (shoemake_matrix, mmc_widom.hpp).  Host mirror:
// observables.pair_molecules.
__device__ __forceinline__ void pair_draw(uint64_t seed, uint64_t ctr, uint32_t replica, double nh[3], double Rm[3][3])
{
    const ChainKey ck{ seed, replica };
    const Uniform2 d3 = mmc_draw(ck, ctr, MMC_WIDOM_SLOT + 3), d4 = mmc_draw(ck, ctr, MMC_WIDOM_SLOT + 4),
                   d5 = mmc_draw(ck, ctr, MMC_WIDOM_SLOT + 5);
    const double z = 1.0 - 2.0 * d3.a, s = sqrt(1.0 - z * z);
    double sp, cp;
    sincos(MMC_TWOPI * d3.b, &sp, &cp);
    nh[0] = s * cp;
    nh[1] = s * sp;
    nh[2] = z;
    shoemake_matrix(d4.a, d4.b, d5.a, Rm);
}

// grid: any number of workgroups of WV_WAVES waves; wave w of workgroup g takes units
// g * WV_WAVES + w, + gridDim.x * WV_WAVES, ... (k_move_eval_wave's map).  Unit u = insertion
// u % M of replica u / M.  The host launches SMAX = 0 when both solutes are uncharged, else 16.
template <int SMAX>
__global__ __launch_bounds__(WV_WAVES * 64) __attribute__((amdgpu_waves_per_eu(SOL_OCC(SMAX), SOL_OCC(SMAX)))) void k_solute_pair_wave(
    BatchView bv, const double *__restrict__ rec, const double *__restrict__ qq_tab,
    const int32_t *__restrict__ kpack, FastConsts fc, PairParams pp, SolutePairArgs sa, int n_units)
{
    constexpr bool QQ = SMAX > 0;
    __shared__ __align__(16) PairShared<SMAX> sm;
    const int tid = threadIdx.x, lane0 = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int SA = sa.n_a, SB = sa.n_b, K = sa.n_sep;
    const int nwa = 3 * SA + 3, nwb = 3 * SB + 3, nrow = 1 + 2 * K;
    if constexpr (QQ)
        for (int k = tid; k < MMC_QQ_TABLE_DOUBLES; k += WV_WAVES * 64)
            sm.qtab[k] = qq_tab[k];
    for (int k = tid; k < (SA + SB) * SOL_PAR; k += WV_WAVES * 64)
        (&sm.par[0][0])[k] = sa.par[k];
    __syncthreads(); // the only workgroup barrier
    const int n_mol = bv.n_mol, nkv = bv.nkvecs;
    const double box = bv.box;
    const BoxConsts bc = box_consts(box);
    const double inv_box = 1.0 / box;
    const uint32_t gate_q = com_quant_gate(fmax(pp.lj_gate_sq, pp.qq_gate_sq), box);
    wv_list_t *const list = sm.list[wv];
    double *const mol = sm.mol[wv];
    double *const tile = pair_tile(sm, wv);
    const int M = sa.n_insert;
    (void)nkv; (void)kpack; (void)fc;

    UNIT_FOR(unit) {
        const int lane = unit_lane(lane0);
        const int r = unit / M, jins = unit - r * M;
        const double *const myrec = rec + (int64_t)r * n_mol * MMC_RSTRIDE;
        double *const trow = sa.terms + (int64_t)unit * nrow * 3;
        uint8_t *const frow = sa.flags + (int64_t)unit * (1 + K);

        // ---- A: word t of [S_A + 1][3] (sites, then c) in lane t, k_solute_wave's expressions;
        // B's frame: word t of [S_B + 1][3] = R_B off_b per site, then the ray's direction ----
        double mwa = 0.0, fwb = 0.0;
        if (sa.mol_a_in) {
            if (lane < nwa)
                mwa = sa.mol_a_in[(int64_t)unit * nwa + lane];
        } else {
            {
                double com[3], Rm[3][3];
                widom_draw(sa.seed, (uint64_t)(sa.draw0 + jins), (uint32_t)r, box, com, Rm);
                const int t = lane < 3 * SA ? lane : 0, a = t / 3, d = t - 3 * a;
                const double r0 = d == 0 ? Rm[0][0] : d == 1 ? Rm[1][0] : Rm[2][0];
                const double r1 = d == 0 ? Rm[0][1] : d == 1 ? Rm[1][1] : Rm[2][1];
                const double r2 = d == 0 ? Rm[0][2] : d == 1 ? Rm[1][2] : Rm[2][2];
                const double o0 = sm.par[a][0], o1 = sm.par[a][1], o2 = sm.par[a][2];
                const double c = d == 0 ? com[0] : d == 1 ? com[1] : com[2];
                const double at = c + ((r0 * o0 + r1 * o1) + r2 * o2);
                const int e = lane - 3 * SA;
                mwa = e < 0 ? at : e == 0 ? com[0] : e == 1 ? com[1] : e == 2 ? com[2] : 0.0;
            }
            {
                double nh[3], Rm[3][3];
                pair_draw(sa.seed, (uint64_t)(sa.draw0 + jins), (uint32_t)r, nh, Rm);
                const int t = lane < 3 * SB ? lane : 0, a = t / 3, d = t - 3 * a;
                const double r0 = d == 0 ? Rm[0][0] : d == 1 ? Rm[1][0] : Rm[2][0];
                const double r1 = d == 0 ? Rm[0][1] : d == 1 ? Rm[1][1] : Rm[2][1];
                const double r2 = d == 0 ? Rm[0][2] : d == 1 ? Rm[1][2] : Rm[2][2];
                const double o0 = sm.par[SA + a][0], o1 = sm.par[SA + a][1], o2 = sm.par[SA + a][2];
                const double ro = (r0 * o0 + r1 * o1) + r2 * o2;
                const int e = lane - 3 * SB;
                fwb = e < 0 ? ro : e == 0 ? nh[0] : e == 1 ? nh[1] : e == 2 ? nh[2] : 0.0;
            }
        }
        if (lane < nwa) {
            if (sa.mol_a_out)
                sa.mol_a_out[(int64_t)unit * nwa + lane] = mwa;
            mol[lane] = mwa;
        }
        if (!sa.mol_a_in && lane < nwb)
            mol[nwa + lane] = fwb;
        wave_sync();

        // word t < nwb of B at separation k: c_B = wrap(c_A + d_k nh) per axis (boundaries.jl:16-26),
        // site b = c_B + R_B off_b -- or the caller's
        auto b_word = [&](int k, int t) -> double {
            if (sa.mol_b_in)
                return sa.mol_b_in[((int64_t)unit * K + k) * nwb + t];
            const int ax = t % 3;
            const double cb = pbc_wrap(mol[3 * SA + ax] + sa.dsep[k] * mol[nwa + 3 * SB + ax], box);
            return t < 3 * SB ? cb + mol[nwa + t] : cb;
        };

        // ---- reciprocal part: per separation one pass over the k list gives s^A and s^B ----
        if constexpr (QQ) {
            cplx(*const pt)[3][MMC_NKTAB] = sm.ptab[wv];
            if (lane < 3 * SA)
                phase_row_moderate(mwa, box, pt[lane / 3][lane % 3]);
            const double *So = s_buf(bv, r, sa.scur[r]);
            for (int k = 0; k < K; k++) { // wave-uniform
                if (lane < 3 * SB)
                    phase_row_moderate(b_word(k, lane), box, pt[SA + lane / 3][lane % 3]);
                wave_sync();
                double a_a = 0.0, a_b = 0.0, a_x = 0.0;
                unit_k_loop(bv, kpack, So, nkv, lane, [&](double wgt, double2 so, int kx, int ky, int kz) {
                    double ar = 0.0, ai = 0.0, br = 0.0, bi = 0.0;
                    for (int l = 0; l < SA; l++) { // wave-uniform
                        const cplx tn = c_mul_fused(c_mul_fused(pt[l][0][5 + kx], pt[l][1][ky]), pt[l][2][kz]);
                        const double q = sm.par[l][3];
                        ar = fma(q, tn.re, ar);
                        ai = fma(q, tn.im, ai);
                    }
                    for (int l = SA; l < SA + SB; l++) {
                        const cplx tn = c_mul_fused(c_mul_fused(pt[l][0][5 + kx], pt[l][1][ky]), pt[l][2][kz]);
                        const double q = sm.par[l][3];
                        br = fma(q, tn.re, br);
                        bi = fma(q, tn.im, bi);
                    }
                    if (k == 0)
                        a_a = fma(wgt, fma(2.0, fma(so.x, ar, so.y * ai), fma(ar, ar, ai * ai)), a_a);
                    a_b = fma(wgt, fma(2.0, fma(so.x, br, so.y * bi), fma(br, br, bi * bi)), a_b);
                    a_x = fma(wgt, 2.0 * fma(ar, br, ai * bi), a_x); // 2 Re(conj(s^A) s^B)
                });
                const double s_b = wave_sum_rows(a_b), s_x = wave_sum_rows(a_x);
                const double s_a = k == 0 ? wave_sum_rows(a_a) : 0.0;
                if (lane == 0) {
                    if (k == 0)
                        trow[2] = s_a * bv.factor + sa.self_a;
                    trow[3 * (1 + k) + 2] = s_b * bv.factor + sa.self_b;
                    trow[3 * (1 + K + k) + 2] = s_x * bv.factor;
                }
                wave_sync(); // (B's rows are rewritten at the next separation, all rows by the first tile)
            }
        }

        // ---- pair part: placements p = 0 (A), 1 + k (B_k) in tiles of PAIR_TILE ----
        const int P = 1 + K;
        for (int p0 = 0; p0 < P; p0 += PAIR_TILE) {
            const int np = min(PAIR_TILE, P - p0);
            // the tile's placements into LDS: slot s, word t in lane t
            for (int s = 0; s < np; s++) {
                const int p = p0 + s;
                if (p == 0) {
                    if (lane < nwa)
                        tile[lane] = mwa;
                } else if (lane < nwb) {
                    const double w = b_word(p - 1, lane);
                    tile[s * PAIR_STRIDE + lane] = w;
                    if (sa.mol_b_out)
                        sa.mol_b_out[((int64_t)unit * K + (p - 1)) * nwb + lane] = w;
                }
            }
            wave_sync();

            uint32_t cqxy[PAIR_TILE], cqz[PAIR_TILE]; // the 16-bit codes of the tile's reference points
#pragma unroll
            for (int s = 0; s < PAIR_TILE; s++) {
                const int ss = s < np ? s : 0; // (an empty slot repeats slot 0)
                const double *c = tile + ss * PAIR_STRIDE + 3 * (p0 + ss == 0 ? SA : SB);
                cqxy[s] = (uint32_t)com_quant(c[0], inv_box) | (uint32_t)com_quant(c[1], inv_box) << 16;
                cqz[s] = (uint32_t)com_quant(c[2], inv_box);
            }
            double a_lj[PAIR_TILE], a_q[PAIR_TILE]; // this lane's sums over every water it takes
            unsigned long long ovm[PAIR_TILE];      // lanes that saw an overlap
#pragma unroll
            for (int s = 0; s < PAIR_TILE; s++) {
                a_lj[s] = 0.0;
                a_q[s] = 0.0;
                ovm[s] = 0ULL;
            }

            // neighbours list[0 .. cnt): lane n takes neighbour n0 + n, gathers its record once and
            // evaluates every placement of the tile against it
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
#pragma unroll
                    for (int s = 0; s < PAIR_TILE; s++) {
                        if (s >= np) // wave-uniform
                            break;
                        const bool isa = p0 + s == 0;
                        const int S = isa ? SA : SB, pb = isa ? 0 : SA;
                        const double *w = tile + s * PAIR_STRIDE;
                        // the gates, exactly: COM minimum image on the reference's arithmetic
                        // (energy.jl:248-254, ewalds.jl:334-340)
                        const double cx = w[3 * S], cy = w[3 * S + 1], cz = w[3 * S + 2];
                        const double gx = vector1D_abs(cx, t[9], bc), gy = vector1D_abs(cy, t[10], bc),
                                     gz = vector1D_abs(cz, t[11], bc);
                        const double c2 = gx * gx + gy * gy + gz * gz;
                        const bool g = QQ && act && (c2 < pp.qq_gate_sq);
                        const bool l = act && (c2 < pp.lj_gate_sq);
                        if (!wave_any(g || l))
                            continue;
                        for (int a = 0; a < S; a++) { // wave-uniform: the site's words are LDS broadcasts
                            const double *p = sm.par[pb + a];
                            const double ax = w[3 * a], ay = w[3 * a + 1], az = w[3 * a + 2];
#pragma unroll
                            for (int b = 0; b < 3; b++) {
                                const double px = vector1D_abs(ax, t[3 * b], bc), py = vector1D_abs(ay, t[3 * b + 1], bc),
                                             pz = vector1D_abs(az, t[3 * b + 2], bc);
                                const double u = px * px + py * py + pz * pz;
                                if constexpr (QQ) {
                                    const double qq = p[3] * fc.q[b];
                                    const bool ov = g && (u < pp.ovr) && (qq < 0.0); // ewalds.jl:359
                                    ovm[s] |= wave_ballot(ov);
                                    double e = 0.0;
                                    if (g && !ov && u < pp.qq_slack_sq) // :362
                                        e = qq_pair(sm.qtab, u, pp.kappa);
                                    a_q[s] = fma(e, qq, a_q[s]); // :365-367
                                }
                                const double eps = p[4 + b];
                                if (l && u < pp.lj_slack_sq && eps > 0.001) { // energy.jl:270
                                    const double sg = p[7 + b];
                                    const double s2 = sg * sg / u;
                                    const double s6 = s2 * s2 * s2;
                                    const double s12 = s6 * s6;
                                    a_lj[s] += eps * (s12 - s6);
                                }
                            }
                        }
                    }
                }
                wave_sync();
            };

            // COM scan on the 16-bit box fractions (k_solute_wave's): a water is listed when the
            // prefilter of ANY of the tile's placements admits it.  Lane per water, four blocks of 64
            // in flight, survivors appended in ascending j; the index is clamped.
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
                        bool near = false;
#pragma unroll
                        for (int s = 0; s < PAIR_TILE; s++)
                            near = near || com_quant_dist2(fxy[q], fz[q], cqxy[s], cqz[s]) < gate_q;
                        const bool keep = j < n_mol && near;
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

            // ---- the tile's terms and flags (k_solute_wave's arithmetic), and the A-B term of
            // each of its separations: lane per site pair (a, b) = (lane / S_B, lane % S_B) ----
            const bool xact = lane < SA * SB;
            const int xl = xact ? lane : 0, xa = xl / SB, xb = xl - xa * SB;
            const double xe = sa.xpar[3 * xl], xs = sa.xpar[3 * xl + 1], xq = sa.xpar[3 * xl + 2];
#pragma unroll
            for (int s = 0; s < PAIR_TILE; s++) {
                if (s >= np)
                    break;
                const int p = p0 + s;
                const double s_lj = wave_sum_rows(a_lj[s]);
                const double s_q = QQ ? wave_sum_rows(a_q[s]) : 0.0;
                const int ov = ovm[s] != 0ULL;
                if (lane == 0) {
                    double *t = trow + 3 * p;
                    t[0] = (0.0 + s_lj) * 4;                  // energy.jl:289
                    if constexpr (QQ) {
                        double d_real = ov ? 0.0 : 0.0 + s_q; // ewalds.jl:359-360
                        d_real *= bv.factor;                  // ewalds.jl:905
                        t[1] = d_real;
                    } else {
                        t[1] = 0.0;
                        t[2] = 0.0;
                    }
                }
                int ovx = 0;
                if (p > 0) {
                    const double *w = tile + s * PAIR_STRIDE;
                    const double gx = vector1D_abs(mol[3 * SA], w[3 * SB], bc), gy = vector1D_abs(mol[3 * SA + 1], w[3 * SB + 1], bc),
                                 gz = vector1D_abs(mol[3 * SA + 2], w[3 * SB + 2], bc);
                    const double c2 = gx * gx + gy * gy + gz * gz;
                    const bool g = QQ && xact && (c2 < pp.qq_gate_sq);
                    const bool l = xact && (c2 < pp.lj_gate_sq);
                    const double px = vector1D_abs(mol[3 * xa], w[3 * xb], bc), py = vector1D_abs(mol[3 * xa + 1], w[3 * xb + 1], bc),
                                 pz = vector1D_abs(mol[3 * xa + 2], w[3 * xb + 2], bc);
                    const double u = px * px + py * py + pz * pz;
                    double v_lj = 0.0, v_q = 0.0;
                    if constexpr (QQ) {
                        const bool o = g && (u < pp.ovr) && (xq < 0.0);
                        ovx = wave_ballot(o) != 0ULL;
                        double e = 0.0;
                        if (g && !o && u < pp.qq_slack_sq)
                            e = qq_pair(sm.qtab, u, pp.kappa);
                        v_q = e * xq;
                    }
                    if (l && u < pp.lj_slack_sq && xe > 0.001) {
                        const double s2 = xs * xs / u;
                        const double s6 = s2 * s2 * s2;
                        const double s12 = s6 * s6;
                        v_lj = xe * (s12 - s6);
                    }
                    const double x_lj = wave_sum_rows(v_lj);
                    const double x_q = QQ ? wave_sum_rows(v_q) : 0.0;
                    if (lane == 0) {
                        double *t = trow + 3 * (K + p);
                        t[0] = (0.0 + x_lj) * 4;
                        if constexpr (QQ) {
                            double x_real = ovx ? 0.0 : 0.0 + x_q;
                            x_real *= bv.factor;
                            t[1] = x_real;
                        } else {
                            t[1] = 0.0;
                            t[2] = 0.0;
                        }
                    }
                }
                if (lane == 0)
                    frow[p] = (uint8_t)((ov ? MMC_WIDOM_OVERLAP : 0) | (ovx ? PAIR_OVERLAP_AB : 0));
            }
            wave_sync(); // (the tile is refilled, list rewritten)
        }
        wave_sync(); // (mol, list and the phase rows are rewritten by this wave's next unit)
    }
}

// One wave per (replica, column): column 0 is A, column 1 + k is separation k.  The weights of
// blocks of 64 insertions (lane per insertion), then the sums in insertion order, as
// k_widom_reduce.  dU = (lj + real) + recip of a row; dU_AB = (dU_A + dU_B) + x.
//   column 0:     sums[r][0] += w_A;  counts[r][0] += flagged;  flags[.][0] gets bit 1
//   column 1 + k: sums[r][1 + k] += w_B;  sums[r][1 + K + k] += w_AB;  the counts likewise;
//                 flags[.][1 + k] gets bits 1 and 3.  w_AB = 0 when any flag of A or of the entry is set.
// words: [R][2 (1 + 2 K)] 8-byte words per replica: 1 + 2 K sums (double), then 1 + 2 K counts (int64).
__global__ __launch_bounds__(64) void k_pair_reduce(const double *__restrict__ terms, uint8_t *__restrict__ flags, int M,
                                                    int K, double inv_temp, double *words)
{
    __shared__ double wsh[2][64];
    const int r = blockIdx.x, col = blockIdx.y, lane = threadIdx.x;
    const int nrow = 1 + 2 * K;
    const double *t = terms + (int64_t)r * M * nrow * 3;
    uint8_t *f = flags + (int64_t)r * M * (1 + K);
    double *sums = words + (int64_t)r * 2 * nrow;
    long long *counts = reinterpret_cast<long long *>(sums + nrow);
    const int i1 = col == 0 ? 0 : col, i2 = col == 0 ? 0 : K + col; // the slots of the two sums
    double acc1 = sums[i1], acc2 = sums[i2];
    long long cnt1 = 0, cnt2 = 0;
    for (int b = 0; b < M; b += 64) {
        const int i = b + lane;
        const int nb = min(64, M - b);
        double w1 = 0.0, w2 = 0.0;
        int z1 = 0, z2 = 0;
        if (i < M) {
            const double *ti = t + (int64_t)i * nrow * 3;
            uint8_t *fi = f + (int64_t)i * (1 + K);
            const double du_a = (ti[0] + ti[1]) + ti[2];
            const int fl_a = (fi[0] & MMC_WIDOM_OVERLAP) | (isfinite(du_a) ? 0 : MMC_WIDOM_NONFINITE);
            if (col == 0) {
                w1 = fl_a ? 0.0 : exp(-du_a * inv_temp);
                z1 = fl_a != 0;
                fi[0] = (uint8_t)fl_a;
            } else {
                const double *tb = ti + 3 * col, *tx = ti + 3 * (K + col);
                const double du_b = (tb[0] + tb[1]) + tb[2];
                const double x = (tx[0] + tx[1]) + tx[2];
                const double du_ab = (du_a + du_b) + x;
                const int fl_b = (fi[col] & MMC_WIDOM_OVERLAP) | (isfinite(du_b) ? 0 : MMC_WIDOM_NONFINITE);
                const int fl_ab = fl_b | (fi[col] & PAIR_OVERLAP_AB) | (isfinite(du_ab) ? 0 : PAIR_NONFINITE_AB);
                w1 = fl_b ? 0.0 : exp(-du_b * inv_temp);
                z1 = fl_b != 0;
                w2 = (fl_a | fl_ab) ? 0.0 : exp(-du_ab * inv_temp);
                z2 = (fl_a | fl_ab) != 0;
                fi[col] = (uint8_t)fl_ab;
            }
        }
        cnt1 += __popcll(wave_ballot(z1 != 0));
        cnt2 += __popcll(wave_ballot(z2 != 0));
        wsh[0][lane] = w1;
        wsh[1][lane] = w2;
        wave_sync();
#pragma unroll 8
        for (int q = 0; q < nb; q++) {
            acc1 += wsh[0][q];
            acc2 += wsh[1][q];
        }
        wave_sync();
    }
    if (lane == 0) {
        sums[i1] = acc1;
        counts[i1] += cnt1;
        if (col > 0) {
            sums[i2] = acc2;
            counts[i2] += cnt2;
        }
    }
}
