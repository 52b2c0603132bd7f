// mmc_unit.hpp -- what the kernels with one wavefront per (replica, molecule) share: k_widom_wave
// (mmc_widom.hpp), k_deletion_wave (mmc_deletion.hpp) and k_forces_wave (mmc_forces.hpp).  A unit is
// the one-state half of a trial move of k_move_eval_wave (mmc_wave.hpp): the molecule is one
// lane-distributed register `mw` (word t of its record in lane t: atoms 0..8, COM 9..11), its phase
// rows go to the wave's LDS, a lane takes a k-vector against the replica's committed S(k), and the
// pair part gathers the neighbours that pass the COM prefilter.  DESIGN.md, "Unit kernels".
//
// Everything here is inlined into its kernel and keeps the arithmetic of the kernels it was taken
// from, expression by expression (the build has -ffp-contract=off: the bits are those of the source).
#pragma once
#include "mmc_wave.hpp"

#define MMC_WIDOM_OVERLAP 1   // flags of a unit (all three calls): an atom pair overlaps (ewalds.jl:359)
#define MMC_WIDOM_NONFINITE 2 // ... a result is NaN or +-inf

// The prologue of a unit kernel: the erfc table into LDS behind the only workgroup barrier, then the
// launch constants under the names mmc_wave_unit.inc reads.  Uses the kernel's parameters bv, qq_tab
// and pp by name.
#define UNIT_PROLOGUE()                                                                          \
    __shared__ __align__(16) WaveShared sm;                                                      \
    const int tid = threadIdx.x, lane0 = tid & 63;                                               \
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);                                     \
    for (int k = tid; k < MMC_QQ_TABLE_DOUBLES; k += WV_WAVES * 64)                              \
        sm.qtab[k] = qq_tab[k];                                                                  \
    __syncthreads(); /* the only workgroup barrier */                                            \
    const int n_mol = bv.n_mol, nkv = bv.nkvecs;                                                 \
    const double box = bv.box;                                                                   \
    const BoxConsts bc = box_consts(box);                                                        \
    const bool same_gate = pp.lj_gate_sq == pp.qq_gate_sq;                                       \
    const double inv_box = uniform_f64(1.0 / box);                                               \
    uint32_t gate_q;                                                                             \
    asm volatile("v_readfirstlane_b32 %0, %1"                                                    \
                 : "=s"(gate_q)                                                                  \
                 : "v"(com_quant_gate(fmax(pp.lj_gate_sq, pp.qq_gate_sq), box)));                \
    wv_list_t *const list = sm.list[wv]

// The unit loop: any number of workgroups of WV_WAVES waves; wave w of workgroup g takes units
// g * WV_WAVES + w, + gridDim.x * WV_WAVES, ... (k_move_eval_wave's map).
#define UNIT_FOR(unit) for (int unit = blockIdx.x * WV_WAVES + wv; unit < n_units; unit += gridDim.x * WV_WAVES)

// the lane index of a unit, opaque to the optimiser (see k_move_eval_wave)
__device__ __forceinline__ int unit_lane(int lane0)
{
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    return lane;
}

// Molecule i0 of the replica whose records are myrec: word t of its record in lane t.  Every lane
// loads a word of the record's own 128-byte line (no load in a branch); words 12..15 are padding.
__device__ __forceinline__ double unit_load_record(const double *myrec, int i0, int lane)
{
    const double raw = myrec[(int64_t)i0 * MMC_RSTRIDE + (lane & (MMC_RSTRIDE - 1))];
    return lane < MMC_REC ? raw : 0.0;
}

// mw in MoveRec layout, the proposal slot (mmc_wave_unit.inc reads MV_COM_NEW, MV_AT_NEW)
__device__ __forceinline__ double unit_proposal_slot(double mw, int lane)
{
    const int src = (lane >= MV_COM_NEW && lane < MV_COM_NEW + 3) ? 9 + lane - MV_COM_NEW
                    : (lane >= MV_AT_NEW && lane < MV_AT_NEW + 9) ? lane - MV_AT_NEW : 12;
    double w = wave_pick(mw, src);
    if (!(src < 12))
        w = 0.0;
    return w;
}

// The phase rows of the molecule's three atoms (phase_row_moderate, the reference's recurrence) into
// sm.ptab[wv][1]: the row of (atom t / 3, axis t % 3) by lane t < 9.
__device__ __forceinline__ void unit_phase_rows(WaveShared &sm, int wv, double mw, int lane, double box)
{
    const int t = lane < 9 ? lane : 0;
    const double x = wave_pick(mw, t);
    if (lane < 9)
        phase_row_moderate(x, box, sm.ptab[wv][1][t / 3][t % 3]);
    wave_sync();
}

// e_{l,k} = exp(i k . r_l) of atom l from its three rows (ky and kz are stored with their offset of nk = 5)
__device__ __forceinline__ cplx unit_phase(const WaveShared &sm, int wv, int l, int kx, int ky, int kz)
{
    return c_mul_fused(c_mul_fused(sm.ptab[wv][1][l][0][5 + kx], sm.ptab[wv][1][l][1][ky]), sm.ptab[wv][1][l][2][kz]);
}

// Lane per k over the half-space list against So, the replica's committed S(k): per_k(wgt, S_k, kx,
// ky, kz) with wgt = cfac_k.  Lanes past the last k-vector redo the last one with weight zero.
template <class PerK>
__device__ __forceinline__ void unit_k_loop(const BatchView &bv, const int32_t *__restrict__ kpack, const double *So,
                                            int nkv, int lane, PerK per_k)
{
    const int n_it = (nkv + 63) >> 6;
    for (int it = 0; it < n_it; it++) {
        const int k = lane + 64 * it;
        const int kc = min(k, nkv - 1);
        const int kp = kpack[kc];
        const double cf = bv.cfac[kc];
        const double2 so = *reinterpret_cast<const double2 *>(So + 2 * kc);
        const int kx = kp & 15, ky = (kp >> 4) & 15, kz = (kp >> 8) & 15;
        per_k(k < nkv ? cf : 0.0, so, kx, ky, kz);
    }
}

// The reciprocal energy of the molecule mw against the committed S(k) of replica r (S buffer scur),
// left in sm.pvw[wv][0]: sum_k cfac_k (2 Re(conj(S_k) s_k) + SIGN |s_k|^2).  SIGN = +1: the molecule is
// added, |S + s|^2 - |S|^2 (Widom); SIGN = -1: S holds it and it is taken out, |S|^2 - |S - s|^2.
template <int SIGN>
__device__ __forceinline__ void unit_recip_energy(WaveShared &sm, int wv, const BatchView &bv,
                                                  const int32_t *__restrict__ kpack, const FastConsts &fc, int r,
                                                  int scur, double mw, int lane, int nkv, double box)
{
    unit_phase_rows(sm, wv, mw, lane, box);
    const double *So = s_buf(bv, r, scur);
    double a_rec = 0.0;
    unit_k_loop(bv, kpack, So, nkv, lane, [&](double wgt, double2 so, int kx, int ky, int kz) {
        double sr = 0.0, si = 0.0;
#pragma unroll
        for (int l = 0; l < 3; l++) {
            const cplx tn = unit_phase(sm, wv, l, kx, ky, kz);
            sr = fma(fc.q[l], tn.re, sr);
            si = fma(fc.q[l], tn.im, si);
        }
        const double s2 = fma(sr, sr, si * si);
        a_rec = fma(wgt, fma(2.0, fma(so.x, sr, so.y * si), SIGN > 0 ? s2 : -s2), a_rec);
    });
    const double s_rec = wave_sum_rows(a_rec);
    if (lane == 0)
        sm.pvw[wv][0] = s_rec;
    wave_sync(); // (ptab is rewritten by this wave's next unit)
}

// Lane 0 combines the sums of the pair part (sm.outw[wv], one state) and the reciprocal energy
// (sm.pvw[wv][0]) in mmc_combine_parts' arithmetic and stores the unit's three terms and its overlap
// flag (the reduce kernel adds the non-finite bit).  outw and pvw are rewritten by this wave's next unit.
__device__ __forceinline__ void unit_store_terms(WaveShared &sm, int wv, int lane, double factor, double self_d,
                                                 double *t, uint8_t *flag)
{
    wave_sync();
    if (lane == 0) {
        const double *o = sm.outw[wv];
        const int ov = (int)(__double_as_longlong(o[7]) >> 1) & 1;
        const double d_lj = (0.0 + o[1]) * 4;                    // energy.jl:289
        double d_real = ov ? 0.0 : 0.0 + o[5];                   // ewalds.jl:359-360
        d_real *= factor;                                        // ewalds.jl:905
        const double d_rec = sm.pvw[wv][0] * factor + self_d;
        t[0] = d_lj;
        t[1] = d_real;
        t[2] = d_rec;
        *flag = (uint8_t)(ov ? MMC_WIDOM_OVERLAP : 0);
    }
    wave_sync();
}
