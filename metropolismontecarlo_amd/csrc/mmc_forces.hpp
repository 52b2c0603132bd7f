// mmc_forces.hpp -- k_forces_wave: the force on every atom, and the force, torque and virials of every
// molecule, on the wave-per-unit scheme of k_deletion_wave (mmc_deletion.hpp): one wavefront per
// (replica, molecule).
//
// The reference has no forces beyond `fab` in LJ_poly_dU; they are defined (include/mmc_hip.h,
// mmc_batch_forces) as minus the gradient of its own total, potential(..., "ewald")
// (Ewald/energy.jl:946-1032), at fixed neighbour sets: the COM gates and the atom slack decide which
// pairs count and are not differentiated.  A force unit is a deletion unit with vector accumulators:
//   * molecule i's 96-byte record (one coalesced load of its 128-byte line) is the lane-distributed
//     register `mw`, word t in lane t;
//   * the reciprocal part: the phase rows of its three atoms (phase_row_moderate, the reference's
//     recurrence), then lane per k over the half-space list against the replica's committed S(k):
//     nine sums of cfac_k n_d Im(conj(S_k) e_{a,k}), (kx, ky, kz) = n the integer vector;
//   * the pair part is this file's own (mmc_wave_unit.inc sums energies only): the same 16-bit COM
//     prefilter into the wave's LDS list, lane n gathers neighbour n's record, the exact fp64 gate,
//     then the nine atom pairs with one table read, one exp and one reciprocal of r^2 each.  A lane
//     keeps nine force components, the reference's own LJ virial sum and the real-space one;
//   * eleven wave sums (wave_sum_rows_n: fixed order), then F, tau, the virials and tau' I^-1 tau
//     are formed and the rows stored by lane 0.
// k_forces_reduce (a wave per replica) forms the per-replica sums in k_deletion_reduce's order.
// Nothing the chains own is written: coordinates, S(k), flags and step counters are only read.
#pragma once
#include "mmc_deletion.hpp"

#ifndef FORCES_OCC
#define FORCES_OCC 3 // waves per SIMD k_forces_wave is compiled for: 154 VGPRs, no scratch (at 4 it spills)
#endif

struct ForcesArgs {
    const int32_t *sel;  // [n] the selected molecules, 0-based (0, 1, .. N - 1 when the caller selects all)
    double *rows;        // [R][n][9]: F (3), tau (3), w_lj, w_real, t
    double *atom;        // [R][n][9] the forces on the three atoms, or NULL
    uint8_t *flags;      // [R][n]
    const uint8_t *scur; // [R] which S buffer holds the replica's committed S(k)
    int32_t n;           // selected molecules per replica
    int32_t has_mass;
    double mass[3];
    double qqf[9];       // factor * (q_a q_b), the host's product, by atom pair 3a + b
    double qrec[3];      // (factor * (4 pi / L)) * q_a
    double c_exp;        // 2 kappa / sqrt(pi)
    double nk2;          // -(kappa * kappa)
};

#define FORCES_ROW 9

// grid: any number of workgroups of WV_WAVES waves; wave w of workgroup g takes units
// g * WV_WAVES + w, + gridDim.x * WV_WAVES, ... (k_move_eval_wave's map).  Unit u = entry u % n of
// replica u / n.  IMG: exactly k_move_eval_wave's condition (the molecule is one of the batch's own).
template <bool IMG>
__global__ __launch_bounds__(WV_WAVES * 64) __attribute__((amdgpu_waves_per_eu(FORCES_OCC, FORCES_OCC))) void k_forces_wave(
    BatchView bv, const double *__restrict__ rec, const double *__restrict__ qq_tab,
    const int32_t *__restrict__ kpack, FastConsts fc, PairParams pp, ForcesArgs fa, int n_units)
{
    UNIT_PROLOGUE();
    double *const frec = sm.pvw[wv]; // the nine reciprocal sums of the unit
    const int n_sel = fa.n;

    UNIT_FOR(unit) {
        const int lane = unit_lane(lane0);
        const int r = unit / n_sel, ent = unit - r * n_sel;
        const int i0 = __builtin_amdgcn_readfirstlane(fa.sel[ent]);
        const double *const myrec = rec + (int64_t)r * n_mol * MMC_RSTRIDE;

        const double mw = unit_load_record(myrec, i0, lane);

        // ================= reciprocal part: nine sums of cfac n_d Im(conj(S) e_a) =================
        {
            unit_phase_rows(sm, wv, mw, lane, box);
            const double *So = s_buf(bv, r, fa.scur[r]);
            double g[9];
#pragma unroll
            for (int q = 0; q < 9; q++)
                g[q] = 0.0;
            unit_k_loop(bv, kpack, So, nkv, lane, [&](double wgt, double2 so, int kx, int ky, int kz) {
                // the integer vector n of k = 2 pi n / L (ky and kz are stored with their offset of nk = 5)
                const double nx = (double)kx, ny = (double)(ky - 5), nz = (double)(kz - 5);
#pragma unroll
                for (int l = 0; l < 3; l++) {
                    const cplx e = unit_phase(sm, wv, l, kx, ky, kz);
                    // Im(conj(S) e) = S.re e.im - S.im e.re
                    const double wi = wgt * fma(so.x, e.im, -(so.y * e.re));
                    g[3 * l] = fma(wi, nx, g[3 * l]);
                    g[3 * l + 1] = fma(wi, ny, g[3 * l + 1]);
                    g[3 * l + 2] = fma(wi, nz, g[3 * l + 2]);
                }
            });
            // (three sums at a time: the row totals of a sum pass through eight scalar registers)
#pragma unroll
            for (int l = 0; l < 3; l++) {
                double g3[3] = { g[3 * l], g[3 * l + 1], g[3 * l + 2] };
                wave_sum_rows_n<3>(g3);
                g[3 * l] = g3[0];
                g[3 * l + 1] = g3[1];
                g[3 * l + 2] = g3[2];
                __builtin_amdgcn_sched_barrier(0);
            }
            double mine = 0.0;
#pragma unroll
            for (int q = 0; q < 9; q++)
                mine = lane == q ? g[q] : mine;
            if (lane < 9)
                frec[lane] = mine;
            wave_sync(); // (ptab is rewritten by this wave's next unit)
        }

        // ================= pair part =================
        double cc[3];          // the centre of mass of i0
        uint32_t cqxy, cqz;    // ... and its 16-bit box-fraction codes (com_quant), x | y << 16
        {
            const bool is_com = lane >= 9 && lane < 12;
            const int myq = is_com ? (int)com_quant(mw, inv_box) : 0;
#pragma unroll
            for (int d = 0; d < 3; d++)
                cc[d] = lane_f64(mw, 9 + d);
            cqxy = (uint32_t)lane_i32(myq, 9) | (uint32_t)lane_i32(myq, 10) << 16;
            cqz = (uint32_t)lane_i32(myq, 11);
        }
        // per lane, over its neighbours in ascending list order (all of the unit's rounds):
        double f[9];           // the forces on atoms 0..2 of i0
        double a_v = 0.0;      // sum rij . fab of the reference's LJ fab (energy.jl:279-281)
        double a_w = 0.0;      // sum rij . (real-space Coulomb pair force)
#pragma unroll
        for (int q = 0; q < 9; q++)
            f[q] = 0.0;
        unsigned long long ovm = 0; // lanes that saw an overlap

        // ---- neighbours list[0 .. cnt): lane n takes neighbour n0 + n ----
        auto process = [&](int cnt) {
            wave_sync();
            for (int n0 = 0; n0 < cnt; n0 += 64) {
                const int n = n0 + lane;
                const int j = n < cnt ? list[n] : 0; // idle lanes: molecule 0, gates forced off
                const bool act = (n < cnt) && (j != i0); // (the scan lets the molecule itself through)
                double t[MMC_REC];
                const double2 *src = reinterpret_cast<const double2 *>(myrec + (int64_t)j * MMC_RSTRIDE);
#pragma unroll
                for (int q = 0; q < 6; q++) {
                    const double2 v = src[q];
                    t[2 * q] = v.x;
                    t[2 * q + 1] = v.y;
                }
                // the gates, exactly: COM minimum image on the reference's arithmetic (energy.jl:248-254,
                // ewalds.jl:334-340); rij = vector1D(COM_i, COM_j), signed: the virials need it
                double m[3], rij[3];
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    const double d1 = t[9 + d] - cc[d];
                    m[d] = (fabs(d1) < bc.half) ? 0.0 : copysign(1.0, d1);
                    rij[d] = fma(m[d], bc.neg, d1); // == vector1D(cc[d], t[9 + d], bc)
                }
                const double c1 = rij[0] * rij[0] + rij[1] * rij[1] + rij[2] * rij[2];
                const bool gq = act && (c1 < pp.qq_gate_sq);                    // ewalds.jl:340
                const bool gl = same_gate ? gq : (act && (c1 < pp.lj_gate_sq)); // energy.jl:254
                double gsum[3] = { 0.0, 0.0, 0.0 }; // the real-space force of this neighbour on i0's atoms, negated
                // one atom pair (a, b); fa3: the force on atom a
                auto pair1 = [&](int ab, double ax, double ay, double az, double bx, double by, double bz,
                                 double (&fa3)[3]) {
                    const bool qneg = (fc.qneg_mask >> ab) & 1; // uniform
                    // rab = vector1D(ra, rb): with IMG the image of the molecule pair (mmc_wave_unit.inc,
                    // WV_IMG: bit for bit vector1D inside a gate), else per atom pair
                    double p[3];
                    if constexpr (IMG) {
                        p[0] = fma(m[0], bc.neg, bx - ax);
                        p[1] = fma(m[1], bc.neg, by - ay);
                        p[2] = fma(m[2], bc.neg, bz - az);
                    } else {
                        p[0] = vector1D(ax, bx, bc);
                        p[1] = vector1D(ay, by, bc);
                        p[2] = vector1D(az, bz, bc);
                    }
                    const double u = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
                    // opposite charges that close: the overlap (ewalds.jl:359); else inside the slack (:362)
                    const bool ovl = gq && qneg && (u < pp.ovr);
                    const bool on = gq && !ovl && (IMG || u < pp.qq_slack_sq);
                    ovm |= wave_ballot(ovl);
                    const unsigned long long im = wave_ballot(on);
                    double e = qq_table_eval_lanes(sm.qtab, u, im); // erfc(kappa r) / r, 0 where off
                    if (wave_ballot(on && u < MMC_QQ_UMIN) != 0ULL) { // like charges below the table (cold)
                        if (on && u < MMC_QQ_UMIN)
                            e = qq_pair_cold(u, pp.kappa);
                    }
                    const double inv_u = 1.0 / u; // (the one reciprocal of the pair)
                    const double ex = exp(fa.nk2 * u);
                    // factor q_a q_b (erfc(kappa r) / r + 2 kappa / sqrt(pi) exp(-kappa^2 r^2)) / r^2
                    const double cq = on ? fa.qqf[ab] * ((e + fa.c_exp * ex) * inv_u) : 0.0;
                    gsum[0] = fma(cq, p[0], gsum[0]);
                    gsum[1] = fma(cq, p[1], gsum[1]);
                    gsum[2] = fma(cq, p[2], gsum[2]);
                    double c = cq;
                    if ((fc.lj_mask >> ab) & 1) { // uniform (energy.jl:270: eps > 0.001); same r^2
                        const double eps = fc.eps9[ab], sg = fc.sig9[ab];
                        const bool lon = gl && (IMG || u < pp.lj_slack_sq);
                        const double s2 = (sg * sg) * inv_u;
                        const double s6 = s2 * s2 * s2;
                        const double s12 = s6 * s6;
                        const double virab = eps * (2.0 * s12 - s6);
                        // the reference's own fab (energy.jl:280) and its virial sum (:281)
                        const double f0 = p[0] * virab * s2, f1 = p[1] * virab * s2, f2 = p[2] * virab * s2;
                        const double dv = rij[0] * f0 + rij[1] * f1 + rij[2] * f2;
                        a_v += lon ? dv : 0.0;
                        // minus the gradient of 4 eps (s12 - s6): 24 eps (2 s12 - s6) / r^2
                        c += lon ? 24.0 * virab * inv_u : 0.0;
                    }
                    fa3[0] = fma(-c, p[0], fa3[0]);
                    fa3[1] = fma(-c, p[1], fa3[1]);
                    fa3[2] = fma(-c, p[2], fa3[2]);
                };
                // (not unrolled over a, as in mmc_wave_unit.inc: unrolled, the per-pair constants are
                // hoisted into registers and spilled.  The accumulators of atom a are f[0..2]; the
                // nine rotate by three after every a, so three trips leave them in place)
#pragma unroll 1
                for (int a = 0; a < 3; a++) {
                    const double ax = lane_f64(mw, 3 * a), ay = lane_f64(mw, 3 * a + 1), az = lane_f64(mw, 3 * a + 2);
                    double fa3[3] = { f[0], f[1], f[2] };
                    pair1(3 * a, ax, ay, az, t[0], t[1], t[2], fa3);
                    __builtin_amdgcn_sched_barrier(0);
                    pair1(3 * a + 1, ax, ay, az, t[3], t[4], t[5], fa3);
                    __builtin_amdgcn_sched_barrier(0);
                    pair1(3 * a + 2, ax, ay, az, t[6], t[7], t[8], fa3);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int d = 0; d < 3; d++) {
                        f[d] = f[3 + d];
                        f[3 + d] = f[6 + d];
                        f[6 + d] = fa3[d];
                    }
                }
                a_w += (rij[0] * gsum[0] + rij[1] * gsum[1]) + rij[2] * gsum[2];
            }
            wave_sync();
        };

        // ---- COM scan: mmc_wave_unit.inc's, for one state and with no pending commit.  Lane per
        // molecule, survivors appended to the list in ascending j; WV_PF blocks of 64 molecules in
        // flight ahead of the one being tested; nothing is clamped (the arrays end in MMC_CQ_PAD
        // readable bytes, mmc_system.inc) and what lies beyond n_mol is masked where it is counted ----
        {
            const uint16_t *cq_base = bv.comq + (int64_t)r * 3 * bv.cq_stride;
            const char *pxy = reinterpret_cast<const char *>(cq_base);
            const char *pz = reinterpret_cast<const char *>(cq_base + 2 * bv.cq_stride);
            const uint32_t ul4 = 4u * (uint32_t)lane, ul2 = 2u * (uint32_t)lane;
            int base = 0, cnt = 0;
            uint32_t fxy[WV_PF], fz[WV_PF];
#pragma unroll
            for (int b = 0; b < WV_PF; b++) {
                fxy[b] = *reinterpret_cast<const uint32_t *>(pxy + 256 * b + ul4);
                fz[b] = *reinterpret_cast<const uint16_t *>(pz + 128 * b + ul2);
            }
            while (base < n_mol) {
#pragma unroll
                for (int b = 0; b < WV_PF; b++) {
                    const int j = base + lane;
                    const uint32_t xy = fxy[b], z = fz[b];
                    // refill this slot with the block WV_PF further on
                    fxy[b] = *reinterpret_cast<const uint32_t *>(pxy + 256 * (b + WV_PF) + ul4);
                    fz[b] = *reinterpret_cast<const uint16_t *>(pz + 128 * (b + WV_PF) + ul2);
                    const bool keep = com_quant_dist2(xy, z, cqxy, cqz) < gate_q;
                    // lanes past n_mol are masked out of the COUNT only: they lie above every lane that
                    // counts, so what they append lands behind the block's last valid entry (room: the
                    // list is checked with 64 WV_PF slots to spare)
                    const int nv = n_mol - base;
                    const unsigned long long m_end = nv >= 64 ? ~0ULL : (nv > 0 ? (1ULL << nv) - 1ULL : 0ULL);
                    const unsigned long long mk = wave_ballot(keep);
                    if (keep)
                        list[cnt + lanes_below(mk)] = (wv_list_t)j;
                    cnt += __popcll(mk & m_end);
                    base += 64;
                }
                pxy += 256 * WV_PF;
                pz += 128 * WV_PF;
                if (cnt > WV_LIST - 64 * WV_PF) { // no room for another WV_PF blocks: empty the list
                    process(cnt);
                    cnt = 0;
                }
            }
            if (cnt)
                process(cnt);
        }

        // ================= the molecule's rows =================
        double s[11]; // (every lane holds the eleven totals; three sums at a time, as above)
#pragma unroll
        for (int l = 0; l < 3; l++) {
            double f3[3] = { f[3 * l], f[3 * l + 1], f[3 * l + 2] };
            wave_sum_rows_n<3>(f3);
            s[3 * l] = f3[0];
            s[3 * l + 1] = f3[1];
            s[3 * l + 2] = f3[2];
            __builtin_amdgcn_sched_barrier(0);
        }
        {
            double w2[2] = { a_v, a_w };
            wave_sum_rows_n<2>(w2);
            s[9] = w2[0];
            s[10] = w2[1];
        }
        {
            const int ov = ovm != 0ULL;
            double fat[9], d[9];
#pragma unroll
            for (int q = 0; q < 9; q++) {
                fat[q] = s[q] + fa.qrec[q / 3] * frec[q];               // pair part + reciprocal part
                d[q] = vector1D(lane_f64(mw, 9 + q % 3), lane_f64(mw, q), bc); // d_a = vector1D(COM, r_a)
            }
            double F[3], tq[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
                F[k] = (fat[k] + fat[3 + k]) + fat[6 + k];
                // tau = sum_a d_a x f_a, atoms in index order
                tq[k] = ((d[k1] * fat[k2] - d[k2] * fat[k1]) + (d[3 + k1] * fat[3 + k2] - d[3 + k2] * fat[3 + k1]))
                        + (d[6 + k1] * fat[6 + k2] - d[6 + k2] * fat[6 + k1]);
            }
            const double w_lj = s[9] * 24 / 3.0; // energy.jl:289
            const double w_real = s[10] / 3.0;
            double tt = 0.0;
            if (fa.has_mass) { // tau' I^-1 tau, I = sum_a m_a (|d_a|^2 1 - d_a d_a'), the inverse by cofactors
                double ixx = 0, iyy = 0, izz = 0, ixy = 0, ixz = 0, iyz = 0;
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    const double x = d[3 * a], y = d[3 * a + 1], z = d[3 * a + 2], ma = fa.mass[a];
                    ixx += ma * (y * y + z * z);
                    iyy += ma * (x * x + z * z);
                    izz += ma * (x * x + y * y);
                    ixy -= ma * (x * y);
                    ixz -= ma * (x * z);
                    iyz -= ma * (y * z);
                }
                const double c00 = iyy * izz - iyz * iyz, c01 = ixz * iyz - ixy * izz, c02 = ixy * iyz - ixz * iyy;
                const double c11 = ixx * izz - ixz * ixz, c12 = ixy * ixz - ixx * iyz, c22 = ixx * iyy - ixy * ixy;
                const double det = (ixx * c00 + ixy * c01) + ixz * c02;
                const double v0 = (c00 * tq[0] + c01 * tq[1]) + c02 * tq[2];
                const double v1 = (c01 * tq[0] + c11 * tq[1]) + c12 * tq[2];
                const double v2 = (c02 * tq[0] + c12 * tq[1]) + c22 * tq[2];
                tt = ((tq[0] * v0 + tq[1] * v1) + tq[2] * v2) / det;
            }
            bool fin = isfinite(w_lj) && isfinite(w_real) && isfinite(tt);
#pragma unroll
            for (int q = 0; q < 9; q++)
                fin = fin && isfinite(fat[q]);
#pragma unroll
            for (int k = 0; k < 3; k++)
                fin = fin && isfinite(F[k]) && isfinite(tq[k]);
            const int fl = (ov ? MMC_WIDOM_OVERLAP : 0) | (fin ? 0 : MMC_WIDOM_NONFINITE);
            if (lane == 0) { // a flagged molecule has zeros in every row
                double *o = fa.rows + (int64_t)unit * FORCES_ROW;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    o[k] = fl ? 0.0 : F[k];
                    o[3 + k] = fl ? 0.0 : tq[k];
                }
                o[6] = fl ? 0.0 : w_lj;
                o[7] = fl ? 0.0 : w_real;
                o[8] = fl ? 0.0 : tt;
                if (fa.atom) {
                    double *oa = fa.atom + (int64_t)unit * 9;
#pragma unroll
                    for (int q = 0; q < 9; q++)
                        oa[q] = fl ? 0.0 : fat[q];
                }
                fa.flags[unit] = (uint8_t)fl;
            }
        }
        wave_sync(); // frec and the list are rewritten by this wave's next unit
    }
}

struct ForcesReduceArgs {
    const double *rows;   // [R][n][9]
    const uint8_t *flags; // [R][n]
    double *fsum;         // [R][9]
    long long *n_flag;    // [R] in / out
    int32_t n, R;
};

// One wave per replica (workgroup g takes replicas g, g + gridDim.x, ...), k_deletion_reduce's order:
// lane l takes the replica's entries l, l + 64, ... in that order and adds, for an unflagged entry,
// 1.0, F.F, tau.tau, t, F_x, F_y, F_z, w_lj and w_real to its nine sums -- every product
// (x x + y y) + z z, unfused -- then the 64 lane sums by wave_sum_rows (DPP, fixed order): the bits
// do not depend on the launch.
__global__ __launch_bounds__(64) void k_forces_reduce(ForcesReduceArgs ra)
{
    const int lane = threadIdx.x;
    const int n = ra.n;
    for (int r = blockIdx.x; r < ra.R; r += gridDim.x) {
        const double *t = ra.rows + (int64_t)r * n * FORCES_ROW;
        const uint8_t *fl = ra.flags + (int64_t)r * n;
        double a[9] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
        double nf = 0.0; // flagged entries of this lane (exact: integers below 2^31)
        for (int e = lane; e < n; e += 64) {
            if (fl[e]) {
                nf += 1.0;
                continue;
            }
            const double *o = t + (int64_t)e * FORCES_ROW;
            const double fx = o[0], fy = o[1], fz = o[2], tx = o[3], ty = o[4], tz = o[5];
            a[0] += 1.0;
            a[1] += (fx * fx + fy * fy) + fz * fz;
            a[2] += (tx * tx + ty * ty) + tz * tz;
            a[3] += o[8];
            a[4] += fx;
            a[5] += fy;
            a[6] += fz;
            a[7] += o[6];
            a[8] += o[7];
        }
        double s[9];
#pragma unroll
        for (int q = 0; q < 9; q++)
            s[q] = wave_sum_rows(a[q]);
        const double nfs = wave_sum_rows(nf);
        if (lane == 0) {
            if (ra.fsum) {
#pragma unroll
                for (int q = 0; q < 9; q++)
                    ra.fsum[9 * (int64_t)r + q] = s[q];
            }
            ra.n_flag[r] += (long long)nfs;
        }
    }
}
