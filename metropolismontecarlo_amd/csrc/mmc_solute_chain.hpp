// mmc_solute_chain.hpp -- one rigid solute held FIXED at the same place in every replica of a batch
// (include/mmc_hip.h, "A fixed solute"): the chains feel it as molecule N + 1 of the reference's
// potential(..., "ewald"), with the definitions of k_solute_wave (mmc_solute.hpp) -- the COM gate on
// the solute's reference point c, the per-pair vector1D image, r^2 < r_cut^2 + 100 and eps > 0.001,
// the batch's erfc table, the overlap rule r^2 < 0.5 and q_a q_b < 0.  The solute never moves, so it
// needs no commit, and by translation invariance one fixed solute is all a solution at infinite
// dilution needs.  Its whole effect on a water's trial move is one more pair term and a constant in
// S(k); the move kernels are not touched:
//   k_solute_move   per (replica, step): the moved water's old and new state against the S sites ->
//                   one more PartOut of that replica (recip = 0), which the host adds to the move
//                   kernel's records (mmc_combine_parts).
//   k_solute_sofk   S_sol(k) = sum_a q_a exp(2 pi i k . r_a / L) by the reference's phase recurrence,
//                   added to both S buffers of every replica after RecipLong: the move kernels'
//                   incremental updates then carry S(k) of the N + 1 system without knowing it.
//   k_solute_total  per replica: the water-solute LJ, virial and real-space sums and the overlap flag.
//   k_rdf_solute    solute-water pair histograms, from c and from every site, against the three water
//                   slots, in mmc_batch_rdf_sites' arithmetic.
//   k_hydration_map the solute-centred 3-D maps: where the waters' sites sit around the solute, which
//                   way the waters point there and what each place adds to the water-solute energy
//                   (at the end of this file).
// One site against one water is solute_site_water(), the same for the moves and the totals.
//
// Lane layout of k_solute_move: a row of 16 lanes per replica, lane a of the row = site a, four
// replicas per wave; a lane runs 2 states x 3 water atoms.  The six sums of a row are an inclusive DPP
// scan inside the row (the first half of wave_sum_rows): fixed order, no LDS, no other row involved,
// so a replica's record does not depend on the launch's range.  A one-site solute leaves 15 of 16
// lanes idle -- the kernel is a few microseconds per launch either way ("A fixed solute").
#pragma once
#include "mmc_solute.hpp"
#include "mmc_struct.hpp"
#include "mmc_sdf.hpp"

#define SOLC_BLOCK 256                     // threads per workgroup of k_solute_move: 16 replicas
#define SOLC_PAR_DOUBLES (SOL_MAX_SITES * SOL_PAR + 4) // device block: [S][SOL_PAR], then c at [16 * SOL_PAR]
#define SOLC_C (SOL_MAX_SITES * SOL_PAR)   // offset of the reference point in the block
#define SOLC_WAVES 4                       // waves per workgroup of k_solute_total / k_rdf_solute

// The solute as the kernels take it: par[a] = position (3), charge, eps (3), sig (3) of site a against
// the three water slots (the SOL_PAR layout of k_solute_wave with the position where it keeps the
// body offset), then the reference point.
struct SoluteView {
    const double *par; // [SOLC_PAR_DOUBLES], device memory
    int32_t n_sites;
    int32_t charged;   // some charge is not zero: the real-space part and S(k) exist
};

struct SolAcc {
    double lj, vir, qq; // raw sums: sum eps (s12 - s6), sum rij . f, sum q_a q_b erfc(kappa r) / r
    bool ov;
};

// Site p of the solute against the water w (atoms w[0..8], centre of mass w[9..11]), the water being
// the CHOSEN molecule of LJ_poly_dU / EwaldReal (energy.jl:209-290, ewalds.jl:293-376) and the solute
// molecule j: rij = vector1D(com_water, c), an atom pair's vector = vector1D(atom_water, site).  (With
// the solute chosen both vectors change sign and every product keeps its bits.)
__device__ __forceinline__ void solute_site_water(const double *__restrict__ p, double cx, double cy, double cz,
                                                  const double *w, const double *__restrict__ qtab, const FastConsts &fc,
                                                  const PairParams &pp, bool charged, const BoxConsts &bc, SolAcc &acc)
{
    const double gx = vector1D(w[9], cx, bc), gy = vector1D(w[10], cy, bc), gz = vector1D(w[11], cz, bc);
    const double c2 = gx * gx + gy * gy + gz * gz;
    const bool g = charged && (c2 < pp.qq_gate_sq); // ewalds.jl:334-340
    const bool l = c2 < pp.lj_gate_sq;              // energy.jl:248-254
    if (!(g || l))
        return;
    const double ax = p[0], ay = p[1], az = p[2];
#pragma unroll
    for (int b = 0; b < 3; b++) {
        const double rx = vector1D(w[3 * b], ax, bc), ry = vector1D(w[3 * b + 1], ay, bc), rz = vector1D(w[3 * b + 2], az, bc);
        const double u = rx * rx + ry * ry + rz * rz;
        if (g) {
            const double qq = p[3] * fc.q[b];
            if ((u < pp.ovr) && (qq < 0.0)) // ewalds.jl:359
                acc.ov = true;
            else if (u < pp.qq_slack_sq)    // :362
                acc.qq = fma(qq_pair(qtab, u, pp.kappa), qq, acc.qq);
        }
        const double eps = p[4 + b];
        if (l && u < pp.lj_slack_sq && eps > 0.001) { // energy.jl:270
            const double sg = p[7 + b];
            const double s2 = sg * sg / u;
            const double s6 = s2 * s2 * s2;
            const double s12 = s6 * s6;
            acc.lj += eps * (s12 - s6);
            const double virab = eps * (2.0 * s12 - s6);
            const double f0 = rx * virab * s2, f1 = ry * virab * s2, f2 = rz * virab * s2;
            acc.vir += gx * f0 + gy * f1 + gz * f2;
        }
    }
}

// inclusive sum over the 16 lanes of a row; lane 15 of the row holds the row's total
__device__ __forceinline__ double row16_scan(double v)
{
    v += dpp_row_shr_f64<1>(v);
    v += dpp_row_shr_f64<2>(v);
    v += dpp_row_shr_f64<4>(v);
    v += dpp_row_shr_f64<8>(v);
    return v;
}

// grid: ceil(nr / 16) workgroups of SOLC_BLOCK threads.  moves: the step's records of ALL replicas (a
// ring slot, or the host-proposal buffer); out: [R] records, replica r's at out[r].
__global__ __launch_bounds__(SOLC_BLOCK) void k_solute_move(SoluteView sv, const MoveRec *__restrict__ moves,
                                                            const double *__restrict__ qq_tab, FastConsts fc, PairParams pp,
                                                            double box, PartOut *out, int r0, int nr, unsigned stamp)
{
    __shared__ __align__(16) double comb[SOLC_BLOCK / 16][8];
    const int tid = threadIdx.x, a = tid & 15, row = tid >> 4;
    const int k = blockIdx.x * (SOLC_BLOCK / 16) + row;
    const bool live = k < nr;
    const int r = r0 + (live ? k : nr - 1); // (an idle row reads the last replica's record and writes nothing)
    const bool site = a < sv.n_sites;
    const double *p = sv.par + SOL_PAR * (site ? a : 0);
    const double cx = sv.par[SOLC_C], cy = sv.par[SOLC_C + 1], cz = sv.par[SOLC_C + 2];
    const BoxConsts bc = box_consts(box);
    const MoveRec *mv = moves + r;
    SolAcc acc[2] = { { 0.0, 0.0, 0.0, false }, { 0.0, 0.0, 0.0, false } };
#pragma unroll
    for (int st = 0; st < 2; st++) {
        double w[12];
#pragma unroll
        for (int q = 0; q < 9; q++)
            w[q] = st ? mv->atoms_new[q] : mv->atoms_old[q];
#pragma unroll
        for (int q = 0; q < 3; q++)
            w[9 + q] = st ? mv->com_new[q] : mv->com_old[q];
        if (site)
            solute_site_water(p, cx, cy, cz, w, qq_tab, fc, pp, sv.charged != 0, bc, acc[st]);
    }
    const double s0 = row16_scan(acc[0].lj), s1 = row16_scan(acc[1].lj), s2 = row16_scan(acc[0].vir),
                 s3 = row16_scan(acc[1].vir), s4 = row16_scan(acc[0].qq), s5 = row16_scan(acc[1].qq);
    const unsigned long long m0 = wave_ballot(acc[0].ov), m1 = wave_ballot(acc[1].ov);
    const int sh = 16 * ((tid & 63) >> 4);
    if (a == 15) {
        double *w8 = comb[row];
        w8[0] = s0; w8[1] = s1; w8[2] = s2; w8[3] = s3; w8[4] = s4; w8[5] = s5;
        w8[6] = 0.0; // no reciprocal part: the solute's S(k) is a constant of the chain
        w8[7] = pack_ovl((int)((m0 >> sh) & 0xffffULL) != 0, (int)((m1 >> sh) & 0xffffULL) != 0, stamp,
                         part_checksum(w8, stamp));
    }
    __syncthreads();
    if (live)
        store_part(out + r, comb[row], a);
}

// grid: R workgroups of MMC_BLOCK threads.  Phase rows of the S sites (ewalds.jl:564-585), then thread
// t takes the k-vectors t, t + MMC_BLOCK, ...: s_k = sum_a q_a e_x e_y e_z in site order from 0, added
// to BOTH buffers of the replica (the state RecipLong leaves: ewalds.jl:600-601).
__global__ __launch_bounds__(MMC_BLOCK) void k_solute_sofk(BatchView bv, SoluteView sv)
{
    __shared__ cplx tab[SOL_MAX_SITES][3][MMC_NKTAB];
    const int tid = threadIdx.x, r = blockIdx.x, S = sv.n_sites;
    if (tid < 3 * S)
        phase_row(sv.par[SOL_PAR * (tid / 3) + tid % 3], bv.box, tab[tid / 3][tid % 3]);
    __syncthreads();
    double *s0 = s_buf(bv, r, 0), *s1 = s_buf(bv, r, 1);
    for (int k = tid; k < bv.nkvecs; k += MMC_BLOCK) {
        const int kx = bv.kxyz[3 * k], ky = bv.kxyz[3 * k + 1], kz = bv.kxyz[3 * k + 2];
        double sr = 0.0, si = 0.0;
        for (int l = 0; l < S; l++) {
            const cplx tn = c_mul(c_mul(tab[l][0][5 + kx], tab[l][1][5 + ky]), tab[l][2][5 + kz]);
            const double q = sv.par[SOL_PAR * l + 3];
            sr += q * tn.re;
            si += q * tn.im;
        }
        s0[2 * k] += sr; s0[2 * k + 1] += si;
        s1[2 * k] += sr; s1[2 * k + 1] += si;
    }
}

// A wave per replica (wave w of workgroup g takes the replicas g * SOLC_WAVES + w, + gridDim.x *
// SOLC_WAVES, ...): lane l adds the waters l, l + 64, ... in that order, each against the sites
// 0 .. S - 1 in order, then the 64 lane sums are added by wave_sum_rows (fixed order): the bits do not
// depend on the launch.
// out[r][4] = sum eps (s12 - s6), sum rij . f, sum q q erfc / r (raw, as a PartOut holds them), overlap (0 / 1).
__global__ __launch_bounds__(SOLC_WAVES * 64) void k_solute_total(BatchView bv, const double *__restrict__ rec,
                                                                  SoluteView sv, const double *__restrict__ qq_tab,
                                                                  FastConsts fc, PairParams pp, double *out, int R)
{
    const int lane = threadIdx.x & 63;
    const int S = sv.n_sites;
    const double cx = sv.par[SOLC_C], cy = sv.par[SOLC_C + 1], cz = sv.par[SOLC_C + 2];
    const BoxConsts bc = box_consts(bv.box);
    // (whole waves leave the loop together: no barrier anywhere)
    for (int r = blockIdx.x * SOLC_WAVES + (threadIdx.x >> 6); r < R; r += gridDim.x * SOLC_WAVES) {
        SolAcc acc = { 0.0, 0.0, 0.0, false };
        for (int j = lane; j < bv.n_mol; j += 64) {
            double w[12];
            load_sites12<true>(bv, rec, r, j, w);
            for (int a = 0; a < S; a++)
                solute_site_water(sv.par + SOL_PAR * a, cx, cy, cz, w, qq_tab, fc, pp, sv.charged != 0, bc, acc);
        }
        const double s_lj = wave_sum_rows(acc.lj), s_v = wave_sum_rows(acc.vir), s_q = wave_sum_rows(acc.qq);
        const bool ov = wave_any(acc.ov);
        if (lane == 0) {
            double *o = out + 4 * (int64_t)r;
            o[0] = s_lj; o[1] = s_v; o[2] = s_q; o[3] = ov ? 1.0 : 0.0;
        }
    }
}

struct RdfSoluteArgs {
    const double *thr;        // [numbins + 2] (rdf_thresholds, mmc_units.inc)
    unsigned long long *hist; // [1 + S][3][numbins] or [R][1 + S][3][numbins], zeroed by the host
    int32_t numbins, per_replica;
    float inv_dr;
    int32_t R;
};

// A workgroup per replica (workgroup g takes the replicas g, g + gridDim.x, ...), thread per water (t,
// t + 256, ...), one row of the histogram at a time: row 0 from the reference point c, row 1 + a from
// site a, each against the three water slots.  d = (solute point) - (water site), its image and the
// bin exactly as k_rdf_sites_wave (st_image, tile_bin on the host's thresholds); a distance in bin
// 1 <= bin <= numbins is counted at [bin - 1].  The row's counters [3][numbins] are 32-bit words in LDS
// (24 KiB at the 2046 bins allowed; a replica adds at most n_mol < 2^31 to a counter), flushed after every replica with one global 64-bit atomic per counter
// that is not zero, as k_rdf_sites_wave flushes its waves' rows.  The counts are integers: any grid
// gives the same.  Dynamic LDS: 12 numbins bytes.
__global__ __launch_bounds__(SOLC_WAVES * 64) void k_rdf_solute(BatchView bv, const double *__restrict__ rec,
                                                                SoluteView sv, RdfSoluteArgs ra)
{
    extern __shared__ unsigned rs_row[]; // [3][numbins]
    const int tid = threadIdx.x;
    const int S = sv.n_sites, nb = ra.numbins;
    const double half = bv.box / 2.0, neg_box = -bv.box;
    const float e_max = (float)(nb + 1);
    for (int r = blockIdx.x; r < ra.R; r += gridDim.x) {
        unsigned long long *h = ra.hist + (ra.per_replica ? (int64_t)r * (1 + S) * 3 * nb : 0);
        for (int row = 0; row <= S; row++) { // (uniform over the workgroup: the barriers are reached by all)
            for (int q = tid; q < 3 * nb; q += SOLC_WAVES * 64)
                rs_row[q] = 0u;
            __syncthreads();
            const double *p = row == 0 ? sv.par + SOLC_C : sv.par + SOL_PAR * (row - 1);
            const double px = p[0], py = p[1], pz = p[2];
            for (int j = tid; j < bv.n_mol; j += SOLC_WAVES * 64) {
                double w[9];
                load_sites9<true>(bv, rec, r, j, w);
#pragma unroll
                for (int b = 0; b < 3; b++) {
                    const double xx = st_image(px - w[3 * b], half, neg_box), yy = st_image(py - w[3 * b + 1], half, neg_box),
                                 zz = st_image(pz - w[3 * b + 2], half, neg_box);
                    const int bin = tile_bin(ra.thr, (xx * xx + yy * yy) + zz * zz, ra.inv_dr, e_max);
                    if (bin >= 1 && bin <= nb)
                        __hip_atomic_fetch_add(&rs_row[b * nb + (bin - 1)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
            __syncthreads();
            for (int q = tid; q < 3 * nb; q += SOLC_WAVES * 64) {
                const unsigned v = rs_row[q];
                if (v != 0u)
                    atomicAdd(&h[(int64_t)row * 3 * nb + q], (unsigned long long)v);
            }
            __syncthreads();
        }
    }
}

// ---- k_hydration_map: the solute-centred maps of mmc_batch_hydration_map -------------------------------
// The solute is fixed and the same in every replica, so the laboratory frame is its frame: one cube of
// (2 n_half)^3 cells on the laboratory axes, centred on the reference point c, takes the deposits of all
// replicas.  A workgroup of HMAP_THREADS threads takes the replicas g, g + gridDim.x, ... and runs one
// PASS per requested channel over them: thread t the waters t, t + HMAP_THREADS, ..., each water one
// deposit -- 1, Q30 of a component of e_z, or Q20 of its pair energy with the solute -- at the cell of
// one of its sites.  x = st_image(site - c) per component; the cell is sd_cell's (mmc_sdf.hpp: a float
// estimate corrected by two compares against the host's edges in LDS, -1 or n beyond the cube and for a
// NaN, no branch on the cell).  The grid is ONE array of 64-bit words per workgroup in LDS (128 KB at
// MMC_HMAP_MAX_CELLS), added to with workgroup-scope LDS atomics; summed output keeps it across all the
// workgroup's replicas of a pass and flushes its non-zero cells once with 64-bit global atomics,
// per-replica output flushes after every replica.  The two tail slots (the deposits outside the cube;
// the waters left out) are kept per thread, added over the wave at the flush, one global atomic a wave.
// Every sum is of 64-bit integers modulo 2^64: no grid, "wave_wgs", set of channels or order of atomics
// changes a bit.  Dynamic LDS: 8 (2 n_half + 1) + 8 n_cells bytes.
#define HMAP_THREADS 1024       // the largest workgroup: 16 waves, 4 per SIMD, at most 128 VGPRs a lane
#define HMAP_U_MAX 1048576.0    // a water's energy of this magnitude (2^20 K) or beyond is flagged
static_assert(8 * MMC_HMAP_MAX_CELLS == 131072, "MMC_HMAP_MAX_CELLS is what 128 KB of LDS hold");
static_assert(MMC_HMAP_CHANNELS == 8, "channels: three counts, three components of e_z, two energies");

struct HmapArgs {
    const double *edge;        // [2 n_half + 1]: e_k = (double)k * cell, built by the host
    unsigned long long *maps;  // [n_ch][n_cells + 2] or [R][n_ch][n_cells + 2], zeroed by the host
    int32_t n_half, n_cells, channel_mask, per_replica;
    float inv_cell;
    int32_t R;
};

// the sum over the 64 lanes, in every lane (integers: any order)
__device__ __forceinline__ long long hm_wave_sum(long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_xor(v, off, 64);
    return v;
}

// The molecules are read from the 128-byte records `rec`, which a batch with a solute always keeps in
// step (mmc_batch_set_solute).  grid: at most R workgroups of HMAP_THREADS threads.
__global__ __launch_bounds__(HMAP_THREADS) void k_hydration_map(BatchView bv, const double *__restrict__ rec, SoluteView sv,
                                                                const double *__restrict__ qq_tab, FastConsts fc,
                                                                PairParams pp, HmapArgs ha)
{
    extern __shared__ __align__(16) unsigned char hm_lds[];
    const int n_edge = 2 * ha.n_half + 1, n_cells = ha.n_cells, tid = threadIdx.x;
    double *const edge = reinterpret_cast<double *>(hm_lds);
    unsigned long long *const cells = reinterpret_cast<unsigned long long *>(hm_lds + 8 * n_edge);
    tile_prologue(edge, ha.edge, n_edge, cells, n_cells);

    const SdfAxis ax = sd_axis(ha.n_half, false);
    const int S = sv.n_sites, n_mol = bv.n_mol;
    const double cx = sv.par[SOLC_C], cy = sv.par[SOLC_C + 1], cz = sv.par[SOLC_C + 2];
    const BoxConsts bc = box_consts(bv.box);
    const double half = bv.box / 2.0, neg_box = -bv.box;
    const int64_t row_len = (int64_t)n_cells + 2;
    const int n_ch = __popc((unsigned)ha.channel_mask);
    long long t_out = 0, t_left = 0; // of this thread since the last flush

    // the grid and the threads' tails added to one row of the output, and cleared
    auto flush = [&](unsigned long long *dst) {
        __syncthreads();
        for (int q = tid; q < n_cells; q += HMAP_THREADS) {
            const unsigned long long v = cells[q];
            if (v != 0ull) {
                atomicAdd(&dst[q], v);
                cells[q] = 0ull;
            }
        }
        const long long s_out = hm_wave_sum(t_out), s_left = hm_wave_sum(t_left);
        if ((tid & 63) == 0) {
            if (s_out != 0)
                atomicAdd(&dst[n_cells], (unsigned long long)s_out);
            if (s_left != 0)
                atomicAdd(&dst[n_cells + 1], (unsigned long long)s_left);
        }
        t_out = 0;
        t_left = 0;
        __syncthreads();
    };

    int ci = 0; // the channel's row among those requested
    for (int ch = 0; ch < MMC_HMAP_CHANNELS; ch++) { // (ch, r and the branches on them are uniform over the workgroup)
        if (!((ha.channel_mask >> ch) & 1))
            continue;
        for (int r = blockIdx.x; r < ha.R; r += gridDim.x) {
            for (int j = tid; j < n_mol; j += HMAP_THREADS) {
                double sx, sy, sz; // the site whose cell takes the deposit
                long long val = 1;
                bool on = true;    // false: the water is left out and counted in the last slot
                if (ch < 6) {
                    double w[9];
                    load_sites9<true>(bv, rec, r, j, w);
                    sx = ch == 1 ? w[3] : ch == 2 ? w[6] : w[0];
                    sy = ch == 1 ? w[4] : ch == 2 ? w[7] : w[1];
                    sz = ch == 1 ? w[5] : ch == 2 ? w[8] : w[2];
                    if (ch >= 3) { // e_z as sd_molecule (mmc_sdf.hpp) forms it
                        double bb[3];
#pragma unroll
                        for (int d = 0; d < 3; d++)
                            bb[d] = vector1D(w[d], w[3 + d], bc) + vector1D(w[d], w[6 + d], bc);
                        const double nb2 = sd_dot(bb[0], bb[1], bb[2], bb[0], bb[1], bb[2]);
                        const double nb = sqrt(nb2);
                        const double ez = (ch == 3 ? bb[0] : ch == 4 ? bb[1] : bb[2]) / nb;
                        on = nb2 > 0.0 && nb2 < INFINITY; // (false for a NaN)
                        val = (long long)rint(on ? ez * MMC_HMAP_VEC_SCALE : 0.0);
                    }
                } else {
                    double w[12];
                    load_sites12<true>(bv, rec, r, j, w);
                    sx = w[0]; sy = w[1]; sz = w[2];
                    SolAcc acc = { 0.0, 0.0, 0.0, false };
                    for (int a = 0; a < S; a++)
                        solute_site_water(sv.par + SOL_PAR * a, cx, cy, cz, w, qq_tab, fc, pp, sv.charged != 0, bc, acc);
                    const double u_lj = (0.0 + acc.lj) * 4, u_real = bv.factor * (0.0 + acc.qq); // mmc_batch_solute_energy's
                    on = !acc.ov && fabs(u_lj) < HMAP_U_MAX && fabs(u_real) < HMAP_U_MAX; // (false for a NaN)
                    val = (long long)rint(on ? (ch == 6 ? u_lj : u_real) * MMC_HMAP_E_SCALE : 0.0);
                }
                const int ix = sd_cell(edge, ax, st_image(sx - cx, half, neg_box), ha.inv_cell);
                const int iy = sd_cell(edge, ax, st_image(sy - cy, half, neg_box), ha.inv_cell);
                const int iz = sd_cell(edge, ax, st_image(sz - cz, half, neg_box), ha.inv_cell);
                const bool in = (unsigned)ix < (unsigned)ax.n && (unsigned)iy < (unsigned)ax.n && (unsigned)iz < (unsigned)ax.n;
                if (on && in)
                    __hip_atomic_fetch_add(&cells[(ix * ax.n + iy) * ax.n + iz], (unsigned long long)val, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_WORKGROUP);
                t_out += (on && !in) ? val : 0;
                t_left += on ? 0 : 1;
            }
            if (ha.per_replica)
                flush(ha.maps + ((int64_t)r * n_ch + ci) * row_len);
        }
        if (!ha.per_replica)
            flush(ha.maps + (int64_t)ci * row_len);
        ci++;
    }
}
