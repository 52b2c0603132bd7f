// mmc_vperturb.hpp -- kernels of mmc_batch_volume_perturb (include/mmc_hip.h, "Virtual volume
// moves"): potential(..., "ewald") (Ewald/energy.jl:946-1032) of every replica at f = 1 and at up to
// eight test boxes L_k = scale[k] L, kappa_k = alpha / L_k, in one read-only pass.
//
//   k_vp_pairs   grid (tile pairs I <= J, replicas of the chunk): the two 64-molecule record tiles of
//                k_total_pairs are loaded ONCE and stay in LDS; for each box the workgroup writes
//                their rescaled copy (k_rescale's arithmetic, volumeChange.jl:62-80) beside them,
//                stages that box's erfc table and runs k_total_pairs' COM gate, Coulomb pass and LJ
//                pass on it.  One partial per (replica, box, tile pair).
//   k_vp_sum     per (replica, box): the tile-pair partials in index order.
//   k_vp_recip   grid (boxes, replicas): k_recip_long_lds on the rescaled atoms -- phases of
//                2 pi (x + d) / L_k in LDS, the reference's recurrence per (kx, ky) column -- with
//                S(k) kept in LDS too and reduced to sum_k cfac_k |S_k|^2 (ewalds.jl:599) in a fixed
//                order.  Nothing of it reaches the batch.
// wave64, fp64, no MFMA.  Nothing here writes to the batch's arrays.
#pragma once
#include "mmc_total.hpp"

#define VP_MAX_SCALES 8
#define VP_BOXES (VP_MAX_SCALES + 1) // f = 1 first, then the caller's scales

struct VpArgs {
    double f[VP_BOXES], box[VP_BOXES], kappa[VP_BOXES];
    int32_t n_box, r0; // boxes of this call; first replica of this launch's chunk
};

struct VpPart {
    double lj, qq;
    int32_t ovl, _pad;
};

struct VpShared {
    alignas(16) double ti[MMC_TM * MMC_REC]; // the replica's tiles as stored: resident for all boxes
    alignas(16) double tj[MMC_TM * MMC_REC];
    alignas(16) double si[MMC_TM * MMC_REC]; // ... rescaled to the current box; si, sj double as
    alignas(16) double sj[MMC_TM * MMC_REC]; // reduction scratch once the passes are done
    alignas(16) double qtab[MMC_QQ_TABLE_DOUBLES];
    double red[2];
    double qq9[9], ljp_eps[9], ljp_sig[9];
    uint16_t list[MMC_TM * MMC_TM];
    int32_t ljp_ab[9];
    int32_t wcnt[MMC_WAVES];
};
static_assert(2 * MMC_TM * MMC_REC >= 2 * MMC_BLOCK, "the rescaled tiles double as reduction scratch");
static_assert(sizeof(VpShared) <= 64 * 1024, "static LDS");

// k_rescale on one record (volumeChange.jl:62-80): new = old * f and d = new - old per COM
// component, every atom + d.  Unfused (-ffp-contract=off).
__device__ __forceinline__ void vp_scale_record(const double *src, double *dst, double f)
{
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double old = src[9 + c], nw = old * f;
        const double d = nw - old;
        dst[9 + c] = nw;
#pragma unroll
        for (int a = 0; a < 3; a++)
            dst[3 * a + c] = src[3 * a + c] + d;
    }
}

// parts: [chunk replica][box][tile pair]
__global__ __launch_bounds__(MMC_BLOCK) void k_vp_pairs(BatchView bv, const double *rec, const double *tabs,
                                                        FastConsts fc, PairParams pp, VpArgs va,
                                                        const int16_t *tile_pairs, int n_pairs, VpPart *parts)
{
    __shared__ __align__(16) VpShared sm;
    const int rl = blockIdx.y, r = va.r0 + rl, tp = blockIdx.x, tid = threadIdx.x;
    const int n_mol = bv.n_mol;
    const int ti_idx = tile_pairs[2 * tp], tj_idx = tile_pairs[2 * tp + 1];
    const bool diag = ti_idx == tj_idx;
    const int i0 = ti_idx * MMC_TM, j0 = tj_idx * MMC_TM;
    const int ni = min(MMC_TM, n_mol - i0), nj = min(MMC_TM, n_mol - j0);
    const double *myrec = rec + (int64_t)r * n_mol * MMC_RSTRIDE;

    for (int g = tid; g < ni * 6; g += MMC_BLOCK)
        *reinterpret_cast<double2 *>(&sm.ti[2 * g]) = *reinterpret_cast<const double2 *>(
            myrec + (int64_t)(i0 + g / 6) * MMC_RSTRIDE + 2 * (g % 6));
    for (int g = tid; g < nj * 6; g += MMC_BLOCK)
        *reinterpret_cast<double2 *>(&sm.tj[2 * g]) = *reinterpret_cast<const double2 *>(
            myrec + (int64_t)(j0 + g / 6) * MMC_RSTRIDE + 2 * (g % 6));
    if (tid < 9) {
        sm.qq9[tid] = fc.qq9[tid];
        sm.ljp_eps[tid] = fc.ljp_eps[tid];
        sm.ljp_sig[tid] = fc.ljp_sig[tid];
        sm.ljp_ab[tid] = fc.ljp_ab[tid];
    }
    const int w = wave_id();
    const int per_wave = MMC_TM * MMC_TM / MMC_WAVES;
    const int n_ljp = fc.n_ljp;

    for (int kb = 0; kb < va.n_box; kb++) {
        __syncthreads(); // the tiles are loaded; the previous box's scratch and table are read no more
        const double f = va.f[kb], box = va.box[kb], kappa = va.kappa[kb];
        if (tid < ni)
            vp_scale_record(&sm.ti[tid * MMC_REC], &sm.si[tid * MMC_REC], f);
        else if (tid >= MMC_TM && tid - MMC_TM < nj)
            vp_scale_record(&sm.tj[(tid - MMC_TM) * MMC_REC], &sm.sj[(tid - MMC_TM) * MMC_REC], f);
        const double *tab = tabs + (int64_t)kb * MMC_QQ_TABLE_DOUBLES;
        for (int k = tid; k < MMC_QQ_TABLE_DOUBLES; k += MMC_BLOCK)
            sm.qtab[k] = tab[k];
        __syncthreads();

        // ---- COM gate (energy.jl:248-254, ewalds.jl:334-340) in box L_k ----
        const BoxConsts bc = box_consts(box);
        int count = 0;
        for (int it = 0; it < per_wave / 64; it++) {
            const int p = w * per_wave + it * 64 + lane_id();
            const int ii = p >> 6, jj = p & 63;
            int fl = 0;
            if (ii < ni && jj < nj && (!diag || ii < jj)) {
                const double dx = vector1D(sm.si[ii * MMC_REC + 9], sm.sj[jj * MMC_REC + 9], bc);
                const double dy = vector1D(sm.si[ii * MMC_REC + 10], sm.sj[jj * MMC_REC + 10], bc);
                const double dz = vector1D(sm.si[ii * MMC_REC + 11], sm.sj[jj * MMC_REC + 11], bc);
                const double r2 = dx * dx + dy * dy + dz * dz;
                fl = ((r2 < pp.lj_gate_sq) ? 1 : 0) | ((r2 < pp.qq_gate_sq) ? 2 : 0);
            }
            const unsigned long long m = __ballot(fl != 0);
            if (fl)
                sm.list[w * per_wave + count + lanes_below(m)] = (uint16_t)(p | (fl << 12));
            count += __popcll(m);
        }
        if (lane_id() == 0)
            sm.wcnt[w] = count;
        __syncthreads();
        const int c0 = sm.wcnt[0], c1 = sm.wcnt[1], c2 = sm.wcnt[2], c3 = sm.wcnt[3];
        const int total = c0 + c1 + c2 + c3;
        auto entry = [&](int pos) {
            int slot;
            if (pos < c0) slot = pos;
            else if (pos < c0 + c1) slot = per_wave + (pos - c0);
            else if (pos < c0 + c1 + c2) slot = 2 * per_wave + (pos - c0 - c1);
            else slot = 3 * per_wave + (pos - c0 - c1 - c2);
            return (int)sm.list[slot];
        };

        double a_lj = 0.0, a_q = 0.0;
        int n_ovl = 0;
        // ---- Coulomb pass: one lane per (molecule pair, a, b) (ewalds.jl:343-372) ----
        {
            int n = tid / 9, ab = tid - 9 * n;
            for (int g = tid; g < total * 9; g += MMC_BLOCK) {
                const int a = (ab * 11) >> 5, b = ab - 3 * a;
                const int e = entry(n);
                const int ii = (e >> 6) & 63, jj = e & 63;
                const double *pa = &sm.si[ii * MMC_REC + 3 * a], *pb = &sm.sj[jj * MMC_REC + 3 * b];
                const double rx = vector1D(pa[0], pb[0], bc);
                const double ry = vector1D(pa[1], pb[1], bc);
                const double rz = vector1D(pa[2], pb[2], bc);
                const double rab2 = rx * rx + ry * ry + rz * rz;
                const double qq = sm.qq9[ab];
                const bool gq = (e & (2 << 12)) != 0;
                const bool ov = gq && (rab2 < pp.ovr) && (qq < 0); // ewalds.jl:359
                const bool in = gq && !ov && (rab2 < pp.qq_slack_sq);
                double ev = qq_table_eval_clamped(sm.qtab, rab2);
                if (__any(in && rab2 < MMC_QQ_UMIN)) {
                    if (rab2 < MMC_QQ_UMIN) ev = qq_pair(sm.qtab, rab2, kappa);
                }
                a_q += in ? qq * ev : 0.0;
                n_ovl |= ov ? 1 : 0;
                n += 28;
                ab += 4;
                if (ab >= 9) { ab -= 9; n += 1; }
            }
        }
        // ---- LJ pass: atom pairs with eps > 0.001 (energy.jl:257-285), energy only ----
        for (int g = MMC_BLOCK - 1 - tid; g < total * n_ljp; g += MMC_BLOCK) {
            int n = g, p = 0;
            if (n_ljp != 1) {
                n = g / n_ljp;
                p = g - n * n_ljp;
            }
            const int e = entry(n);
            if (e & (1 << 12)) {
                const int ii = (e >> 6) & 63, jj = e & 63;
                const int ab = sm.ljp_ab[p];
                const int a = ab / 3, b = ab - 3 * a;
                const double *ri = &sm.si[ii * MMC_REC], *rj = &sm.sj[jj * MMC_REC];
                const double rx = vector1D(ri[3 * a], rj[3 * b], bc);
                const double ry = vector1D(ri[3 * a + 1], rj[3 * b + 1], bc);
                const double rz = vector1D(ri[3 * a + 2], rj[3 * b + 2], bc);
                const double rab2 = rx * rx + ry * ry + rz * rz;
                if (rab2 < pp.lj_slack_sq) {
                    const double eps = sm.ljp_eps[p], sg = sm.ljp_sig[p];
                    const double s2 = sg * sg / rab2;
                    const double s6 = s2 * s2 * s2;
                    const double s12 = s6 * s6;
                    a_lj += eps * (s12 - s6);
                }
            }
        }
        __syncthreads(); // the rescaled tiles are read no more: reuse them as reduction scratch
        const double v[2] = { a_lj, a_q };
        block_sum_wide<2>(v, sm.si, sm.red, n_ovl, sm.wcnt);
        if (tid == 0) {
            VpPart o;
            o.lj = sm.red[0]; o.qq = sm.red[1];
            o.ovl = (sm.wcnt[0] | sm.wcnt[1] | sm.wcnt[2] | sm.wcnt[3]) & 1;
            o._pad = 0;
            parts[((int64_t)rl * va.n_box + kb) * n_pairs + tp] = o;
        }
    }
}

// sums: [replica][box], replicas r0 .. r0 + n_rep - 1 from this chunk's parts; index order.
__global__ void k_vp_sum(const VpPart *parts, int n_pairs, int n_box, int r0, int n_rep, VpPart *sums)
{
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n_rep * n_box)
        return;
    const VpPart *p = parts + (int64_t)u * n_pairs;
    double lj = 0.0, qq = 0.0;
    int ov = 0;
    for (int k = 0; k < n_pairs; k++) {
        lj += p[k].lj; qq += p[k].qq; ov |= p[k].ovl;
    }
    VpPart o;
    o.lj = lj; o.qq = qq; o.ovl = ov; o._pad = 0;
    sums[(int64_t)r0 * n_box + u] = o;
}

// out[r][box] = sum_k cfac_box[k] |S_k|^2 of replica r's atoms rescaled to that box.  Dynamic LDS:
// [n_atoms][6] phases, [n_atoms] charges, [2 MMC_NK_STRIDE] S(k).
__global__ __launch_bounds__(RL_WAVES * 64) void k_vp_recip(BatchView bv, RecipOrder order, VpArgs va,
                                                            const double *cfac_rows, double *out)
{
    extern __shared__ __align__(16) double vp_lds[];
    __shared__ int next_col;
    __shared__ double red[RL_WAVES];
    const int n_atoms = bv.n_atoms, n_mol = bv.n_mol;
    double *ph = vp_lds;
    double *qv = vp_lds + 6 * n_atoms;
    double *S = vp_lds + 7 * n_atoms + (n_atoms & 1); // 16-byte aligned
    const int kb = blockIdx.x, r = va.r0 + blockIdx.y;
    const double f = va.f[kb], L = va.box[kb];
    if (threadIdx.x == 0)
        next_col = 0;
    for (int j = threadIdx.x; j < n_mol; j += RL_WAVES * 64) {
        const int64_t m = r * bv.mol_stride + j;
        const double com[3] = { bv.comx[m], bv.comy[m], bv.comz[m] };
        double d[3];
#pragma unroll
        for (int c = 0; c < 3; c++) { // k_rescale (volumeChange.jl:62-80)
            const double nw = com[c] * f;
            d[c] = nw - com[c];
        }
        const int fa = bv.first0[j], na = bv.cnt[j];
        for (int a = 0; a < na; a++) {
            const int l = fa + a;
            const int64_t o = r * bv.atom_stride + l;
            double sn, cs;
            sincos_moderate(MMC_TWOPI * (bv.ax[o] + d[0]) / L, sn, cs); ph[6 * l] = cs; ph[6 * l + 1] = sn;
            sincos_moderate(MMC_TWOPI * (bv.ay[o] + d[1]) / L, sn, cs); ph[6 * l + 2] = cs; ph[6 * l + 3] = sn;
            sincos_moderate(MMC_TWOPI * (bv.az[o] + d[2]) / L, sn, cs); ph[6 * l + 4] = cs; ph[6 * l + 5] = sn;
            qv[l] = bv.charge[l];
        }
    }
    __syncthreads();
    const int lane0 = threadIdx.x & 63;
    for (;;) {
        int lane = lane0;
        asm volatile("" : "+v"(lane));
        int slot = 0;
        if (lane == 0)
            slot = atomicAdd(&next_col, 1);
        slot = __builtin_amdgcn_readfirstlane(slot);
        if (slot >= order.n)
            break;
        const int c = order.col[slot];
        const int kx = c / MMC_NKTAB, ky = c % MMC_NKTAB - 5;
        const int16_t *col = bv.kmap + c * MMC_NKTAB;
        int m = 0;
        for (int k = 0; k <= 5; k++)
            if (col[5 + k] >= 0 || col[5 - k] >= 0)
                m = k;
        switch (m) { // (both targets of the column are the one LDS array)
        case 0:
        case 1: recip_column_lds<1>(col, S, S, ph, qv, n_atoms, kx, ky, lane); break;
        case 2: recip_column_lds<2>(col, S, S, ph, qv, n_atoms, kx, ky, lane); break;
        case 3: recip_column_lds<3>(col, S, S, ph, qv, n_atoms, kx, ky, lane); break;
        case 4: recip_column_lds<4>(col, S, S, ph, qv, n_atoms, kx, ky, lane); break;
        default: recip_column_lds<5>(col, S, S, ph, qv, n_atoms, kx, ky, lane); break;
        }
    }
    __syncthreads();
    // ewalds.jl:599 in k_recip_energy's arithmetic: thread t adds k = t, t + 1024, ...; the 64 lanes of
    // a wave by wave_sum, the waves in index order
    const double *cfac = cfac_rows + (int64_t)kb * MMC_NK_STRIDE;
    double v = 0.0;
    for (int k = threadIdx.x; k < bv.nkvecs; k += RL_WAVES * 64) {
        const double re = S[2 * k], im = S[2 * k + 1];
        v += cfac[k] * (re * re - (-im) * im);
    }
    v = wave_sum(v);
    if (lane0 == 0)
        red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int wv = 0; wv < RL_WAVES; wv++)
            s += red[wv];
        out[(int64_t)r * va.n_box + kb] = s;
    }
}
