// mmc_solute_force.hpp -- what the water does to the fixed solute (include/mmc_hip.h,
// mmc_batch_solute_forces): the Lennard-Jones force, the electric field and the electrostatic potential
// at every site of the solute, and the force and torque on it, in every replica.  All of it is the
// gradient of the terms of potential(..., "ewald") of the N + 1 system that depend on the solute, at fixed
// neighbour sets (the COM gates on the reference point c and the atom slack are not differentiated), as
// mmc_batch_forces defines the forces on the waters (mmc_forces.hpp).
//   k_solute_phase  e_{a,k} = exp(2 pi i n_k . r_a / L) of the S sites over the half-space list, by the
//                   reference's phase recurrence (k_solute_sofk's rows and products): the box is shared
//                   and the solute fixed, so ONE table [S][nkvecs] serves every replica of the call.
//   k_solute_force  a wave per replica (k_solute_total's map), the sites one after the other: lane l adds
//                   the waters l, l + 64, ... (atoms 0, 1, 2) into the site's seven pair sums, then the
//                   k-vectors l, l + 64, ... into its four reciprocal sums; the 64 lane sums go through
//                   wave_sum_rows.  The site's row waits in the wave's LDS until the replica's flags are
//                   known (a flagged replica has zeros in every row).
// Site outside, waters inside: a lane keeps eleven accumulators whatever S is (16 sites would be 176
// doubles), and the replica's records (72 KB at 750 waters) are read S times out of L2.
// Nothing the chains own is written.
#pragma once
#include "mmc_solute_chain.hpp"

#define SOLF_ROW 12 // doubles of a site's row in LDS: site_lj (3), field (3), phi, recip (4), one of padding

struct SoluteForceArgs {
    const cplx *etab;    // [S][nkvecs]: k_solute_phase's table
    const uint8_t *scur; // [R] which S buffer holds the replica's committed S(k)
    double *ft;          // [R][6] force, torque                    (any of the outputs may be NULL)
    double *site_lj;     // [R][S][3]
    double *field;       // [R][S][3]
    double *phi;         // [R][S]
    double *recip;       // [R][S][4]
    uint8_t *flags;      // [R]
    double qw[3];        // q_b of the water's three atoms
    double fq[3];        // factor * q_b
    double c_exp;        // 2 kappa / sqrt(pi)
    double nk2;          // -(kappa * kappa)
    double f_rec;        // factor * (4 pi / L)
    double f_phi;        // 2 factor
    double c_self;       // 2 factor kappa / sqrt(pi) (EwaldSelf: ewalds.jl:829-833, differentiated by q_a)
    int32_t R;
};

// grid: one workgroup of MMC_BLOCK threads.  The rows of k_solute_sofk, then thread t takes the k-vectors
// t, t + MMC_BLOCK, ...
__global__ __launch_bounds__(MMC_BLOCK) void k_solute_phase(BatchView bv, SoluteView sv, cplx *etab)
{
    __shared__ cplx tab[SOL_MAX_SITES][3][MMC_NKTAB];
    const int tid = threadIdx.x, S = sv.n_sites;
    if (tid < 3 * S)
        phase_row(sv.par[SOL_PAR * (tid / 3) + tid % 3], bv.box, tab[tid / 3][tid % 3]);
    __syncthreads();
    for (int k = tid; k < bv.nkvecs; k += MMC_BLOCK) {
        const int kx = bv.kxyz[3 * k], ky = bv.kxyz[3 * k + 1], kz = bv.kxyz[3 * k + 2];
        for (int a = 0; a < S; a++)
            etab[(int64_t)a * bv.nkvecs + k] = c_mul(c_mul(tab[a][0][5 + kx], tab[a][1][5 + ky]), tab[a][2][5 + kz]);
    }
}

// A wave per replica (wave w of workgroup g takes the replicas g * SOLC_WAVES + w, + gridDim.x *
// SOLC_WAVES, ...).  Every sum of a replica is formed by its own wave in a fixed order: the bits do not
// depend on the launch, nor on which outputs are asked for.
__global__ __launch_bounds__(SOLC_WAVES * 64) void k_solute_force(BatchView bv, const double *__restrict__ rec,
                                                                  SoluteView sv, const double *__restrict__ qq_tab,
                                                                  PairParams pp, SoluteForceArgs fa)
{
    __shared__ __align__(16) double qtab[MMC_QQ_TABLE_DOUBLES];
    __shared__ double rows[SOLC_WAVES][SOL_MAX_SITES][SOLF_ROW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int k = tid; k < MMC_QQ_TABLE_DOUBLES; k += SOLC_WAVES * 64)
        qtab[k] = qq_tab[k];
    __syncthreads(); // the only workgroup barrier (whole waves leave the loop below together)
    const int S = sv.n_sites, nkv = bv.nkvecs, n_mol = bv.n_mol;
    const double cx = sv.par[SOLC_C], cy = sv.par[SOLC_C + 1], cz = sv.par[SOLC_C + 2];
    const BoxConsts bc = box_consts(bv.box);
    double(*const my)[SOLF_ROW] = rows[wv];

    for (int r = blockIdx.x * SOLC_WAVES + wv; r < fa.R; r += gridDim.x * SOLC_WAVES) {
        const double2 *So = reinterpret_cast<const double2 *>(s_buf(bv, r, fa.scur[r]));
        bool ov = false;
        double F[3] = { 0.0, 0.0, 0.0 }, tq[3] = { 0.0, 0.0, 0.0 };
        bool fin = true;
        for (int a = 0; a < S; a++) { // (uniform)
            const double *__restrict__ p = sv.par + SOL_PAR * a;
            const double ax = p[0], ay = p[1], az = p[2], qa = p[3];
            // ---- pair part: site_lj (3), the real-space field (3) and potential ----
            double lj[3] = { 0.0, 0.0, 0.0 }, pr[4] = { 0.0, 0.0, 0.0, 0.0 }; // pr: field (3), phi
            for (int j = lane; j < n_mol; j += 64) {
                double w[12];
                load_sites12<true>(bv, rec, r, j, w);
                const double gx = vector1D(w[9], cx, bc), gy = vector1D(w[10], cy, bc), gz = vector1D(w[11], cz, bc);
                const double c2 = gx * gx + gy * gy + gz * gz;
                const bool g = c2 < pp.qq_gate_sq; // ewalds.jl:334-340 (charged or not: phi and the field are outputs)
                const bool l = c2 < pp.lj_gate_sq; // energy.jl:248-254
                if (!(g || l))
                    continue;
#pragma unroll
                for (int b = 0; b < 3; b++) {
                    const double rx = vector1D(w[3 * b], ax, bc), ry = vector1D(w[3 * b + 1], ay, bc),
                                 rz = vector1D(w[3 * b + 2], az, bc);
                    const double u = rx * rx + ry * ry + rz * rz;
                    const double inv_u = 1.0 / u;
                    if (g) {
                        if ((u < pp.ovr) && (qa * fa.qw[b] < 0.0)) // ewalds.jl:359
                            ov = true;
                        else if (u < pp.qq_slack_sq) {            // :362
                            const double e = u >= MMC_QQ_UMIN ? qq_table_eval(qtab, u) : qq_pair_cold(u, pp.kappa);
                            const double ex = exp(fa.nk2 * u);
                            // factor q_b (erfc(kappa r) / r + 2 kappa / sqrt(pi) exp(-kappa^2 r^2)) / r^2
                            const double cq = fa.fq[b] * ((e + fa.c_exp * ex) * inv_u);
                            pr[0] += cq * rx;
                            pr[1] += cq * ry;
                            pr[2] += cq * rz;
                            pr[3] += fa.fq[b] * e;
                        }
                    }
                    const double eps = p[4 + b];
                    if (l && u < pp.lj_slack_sq && eps > 0.001) { // energy.jl:270
                        const double sg = p[7 + b];
                        const double s2 = (sg * sg) * inv_u;
                        const double s6 = s2 * s2 * s2;
                        const double s12 = s6 * s6;
                        // minus the gradient of 4 eps (s12 - s6): 24 eps (2 s12 - s6) / r^2
                        const double cl = 24.0 * (eps * (2.0 * s12 - s6)) * inv_u;
                        lj[0] += cl * rx;
                        lj[1] += cl * ry;
                        lj[2] += cl * rz;
                    }
                }
            }
            // ---- reciprocal part: sum_k cfac_k n_k Im(conj(S_k) e_{a,k}), sum_k cfac_k Re(conj(S_k) e_{a,k}) ----
            double g4[4] = { 0.0, 0.0, 0.0, 0.0 };
            const cplx *et = fa.etab + (int64_t)a * nkv;
            for (int k = lane; k < nkv; k += 64) {
                const cplx e = et[k];
                const double2 so = So[k];
                const double wgt = bv.cfac[k];
                const double nx = (double)bv.kxyz[3 * k], ny = (double)bv.kxyz[3 * k + 1], nz = (double)bv.kxyz[3 * k + 2];
                const double wi = wgt * (so.x * e.im - so.y * e.re);
                g4[0] += wi * nx;
                g4[1] += wi * ny;
                g4[2] += wi * nz;
                g4[3] += wgt * (so.x * e.re + so.y * e.im);
            }
            wave_sum_rows_n<3>(lj);
            wave_sum_rows_n<4>(pr);
            wave_sum_rows_n<4>(g4);
            // ---- the site's row (every lane holds the totals) ----
            double rc[4], fld[3], fs[3];
#pragma unroll
            for (int d = 0; d < 3; d++) {
                rc[d] = fa.f_rec * g4[d];
                fld[d] = pr[d] + rc[d];
                fs[d] = lj[d] + qa * fld[d]; // f_a = site_lj[a] + q_a field[a] = -dU/dr_a
            }
            rc[3] = fa.f_phi * g4[3];
            const double ph = (pr[3] + rc[3]) - fa.c_self * qa;
            const double dx = vector1D(cx, ax, bc), dy = vector1D(cy, ay, bc), dz = vector1D(cz, az, bc); // d_a
            F[0] += fs[0];
            F[1] += fs[1];
            F[2] += fs[2];
            tq[0] += dy * fs[2] - dz * fs[1];
            tq[1] += dz * fs[0] - dx * fs[2];
            tq[2] += dx * fs[1] - dy * fs[0];
#pragma unroll
            for (int d = 0; d < 3; d++)
                fin = fin && isfinite(lj[d]) && isfinite(fld[d]) && isfinite(rc[d]);
            fin = fin && isfinite(ph) && isfinite(rc[3]);
            if (lane == 0) {
                double *o = my[a];
                o[0] = lj[0]; o[1] = lj[1]; o[2] = lj[2];
                o[3] = fld[0]; o[4] = fld[1]; o[5] = fld[2];
                o[6] = ph;
                o[7] = rc[0]; o[8] = rc[1]; o[9] = rc[2]; o[10] = rc[3];
            }
        }
#pragma unroll
        for (int d = 0; d < 3; d++)
            fin = fin && isfinite(F[d]) && isfinite(tq[d]);
        const int fl = (wave_any(ov) ? MMC_WIDOM_OVERLAP : 0) | (fin ? 0 : MMC_WIDOM_NONFINITE); // (uniform)
        wave_sync(); // lane 0's rows are read by the others
        // a flagged replica has zeros in every row
        const int64_t r64 = r;
        for (int q = lane; q < 3 * S; q += 64) {
            const int a = q / 3, d = q - 3 * a;
            if (fa.site_lj)
                fa.site_lj[r64 * 3 * S + q] = fl ? 0.0 : my[a][d];
            if (fa.field)
                fa.field[r64 * 3 * S + q] = fl ? 0.0 : my[a][3 + d];
        }
        for (int q = lane; q < 4 * S; q += 64) {
            if (fa.recip)
                fa.recip[r64 * 4 * S + q] = fl ? 0.0 : my[q >> 2][7 + (q & 3)];
        }
        if (lane < S && fa.phi)
            fa.phi[r64 * S + lane] = fl ? 0.0 : my[lane][6];
        if (lane == 0) {
            if (fa.ft) {
                double *o = fa.ft + 6 * r64;
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    o[d] = fl ? 0.0 : F[d];
                    o[3 + d] = fl ? 0.0 : tq[d];
                }
            }
            if (fa.flags)
                fa.flags[r] = (uint8_t)fl;
        }
        wave_sync(); // the rows are rewritten by this wave's next replica
    }
}
