// mmc_voronoi.hpp -- the Voronoi cell of every oxygen, read-only beside the chains:
//   k_voronoi_wave   per molecule: its O-O neighbours inside r_list sorted by distance (up to
//                    MMC_VORONOI_CAP of them), one polygon per neighbour clipped against the other
//                    neighbours' half-planes, and from the polygons the cell's volume, surface,
//                    asphericity, counted faces and flags
//   k_voronoi_sums   the per-replica sums over the per-molecule arrays, in k_local_qsum's order
// The arithmetic is stated in include/mmc_hip.h ("Voronoi cells") and restated in numpy by
// tests/voronoi_ref.py; slot 0 of a molecule is the heavy atom.
//
// The scheme is mmc_nbr.hpp's, as k_shell_order_wave (mmc_shell.hpp): a persistent workgroup takes a contiguous run of
// the R N molecules, stages the O positions of every replica its run touches in LDS (STAGE), and its
// waves take the run's molecules of that replica in turn; inside a molecule a wave waits for nobody.
//
// One molecule i, one wave:
//   scan, sort   scan_list and rank_sort (mmc_nbr.hpp): lane k then owns neighbour k.
//   clip     lane k's polygon lives in LDS, vertex j of lane l at slot 64 j + l (16 bytes a vertex:
//            a wave's lanes read and write consecutive slots).  The planes m = 0, 1, ... come by
//            readlane from the sorted lanes; a lane sits a plane out when it is lane m, has no
//            polygon left or has stopped (the pruning rule of the header); the wave leaves the loop
//            when every lane has.  A clip is one pass over the lane's vertices IN PLACE: the polygon
//            is read into registers first (sixteen independent reads, one wait), then the pass
//            writes the new list over the old one.
//   reduce   the areas by lane, the cell's sums by readlane in rising rank, the flags by ballot.
// Counters: 32-bit, in LDS, one set per workgroup, added to the 64-bit global ones whenever the
// workgroup leaves a replica, as k_shell_order_wave's.  (A workgroup adds at most 64 N faces of one
// replica before that: below 2^32 for the 2^21 molecules allowed.)
//
// Occupancy is set by the LDS: a wave's polygons are 16 KiB, so the 160 KiB of a compute unit hold
// one workgroup of VO_WAVES = 8 waves with its lists, counters and staged positions -- two waves per
// SIMD -- whatever the registers allow ("Voronoi cells").
#pragma once
#include "mmc_shell.hpp"

#define VO_WAVES 8                                   // waves per workgroup (fewer where they would not fit: host)
#define VO_POLY_BYTES (16 * MMC_VORONOI_MAXV * 64)   // a wave's polygons
#define VO_CU_LDS (160 * 1024)                       // the LDS of a compute unit (gfx950)
#define VO_CAP 1
#define VO_OPEN 2
#define VO_POLY 4

struct VoronoiArgs {
    const double *box_r;            // [R] per-replica boxes, or NULL: bv.box
    unsigned long long *flagged;    // [R][3], zeroed by the host
    unsigned long long *vol_hist;   // [v_bins + 1] or [R][..], zeroed by the host; or NULL
    unsigned long long *eta_hist;   // [eta_bins + 1] or [R][..]; or NULL
    unsigned long long *face_hist;  // [65] or [R][65]; or NULL
    unsigned long long *side_hist;  // [17] or [R][17]; or NULL
    unsigned long long *nbr_hist;   // [r_bins + 1] or [R][..]; or NULL
    double *vol, *area, *carea;     // [R][N] or NULL
    int32_t *faces;                 // [R][N] or NULL
    int32_t *nbr;                   // [R][N][64] or NULL
    double *face_area;              // [R][N][64] or NULL
    double rl, rl2, area_min, v_scale, eta_scale, inv_dr, k36pi; // formed by the host
    int32_t v_bins, eta_bins, r_bins;
    int32_t o_eta, o_face, o_side, o_nbr, hs; // the counter words: [0, 3) flagged, [3, o_eta) volumes, ..., hs in all
    int32_t per_replica, R, prune;
};

// (int)floor(x) clamped to [0, top], top where x is not finite
__device__ __forceinline__ int vo_bin(double x, int top)
{
    return __builtin_isfinite(x) ? sh_bin(x, top) : top;
}

// REC, STAGE, grid: as k_shell_order_wave.
// dynamic LDS: [nw] lists of NBR_LIST_BYTES, [nw] polygon sets of VO_POLY_BYTES, [hs] counters, then
// (STAGE) 3 N doubles at the next multiple of 16 bytes.
template <bool REC, bool STAGE>
__global__ __launch_bounds__(VO_WAVES * 64) void k_voronoi_wave(BatchView bv, const double *__restrict__ rec,
                                                                VoronoiArgs va)
{
    extern __shared__ __align__(16) unsigned char vo_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nw = (int)(blockDim.x >> 6);
    const int n_mol = bv.n_mol, hs = va.hs;
    const size_t per_wave = NBR_LIST_BYTES + VO_POLY_BYTES;
    unsigned long long *const keys = reinterpret_cast<unsigned long long *>(vo_lds + (size_t)wv * NBR_LIST_BYTES);
    int *const idx = reinterpret_cast<int *>(keys + MMC_VORONOI_CAP);
    double2 *const poly = reinterpret_cast<double2 *>(vo_lds + (size_t)nw * NBR_LIST_BYTES + (size_t)wv * VO_POLY_BYTES) + lane;
    unsigned *const hw = reinterpret_cast<unsigned *>(vo_lds + (size_t)nw * per_wave); // the workgroup's
    double *const pos = reinterpret_cast<double *>(vo_lds + (((size_t)nw * per_wave + 4 * (size_t)hs + 15) & ~(size_t)15));
    for (int q = tid; q < hs; q += (int)blockDim.x)
        hw[q] = 0u;
    __syncthreads();

    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const double prune_margin = 1.0 + 0x1p-20; // MMC_VORONOI_PRUNE
    const Sites<REC, STAGE> sites{ bv, rec, pos };

    for (RunCursor rc(va.R, n_mol); rc.next();) { // the run's molecules of one replica: [rc.lo, rc.hi) of replica r
        const int r = rc.r;
        if constexpr (STAGE)
            stage_sites(sites, r);
        const BoxConsts bc = box_consts(va.box_r ? va.box_r[r] : bv.box);

        for (int i = rc.lo + wv; i < rc.hi; i += nw) {
            const int64_t g = (int64_t)r * n_mol + i;
            double cx, cy, cz; // the wave's oxygen: wave-uniform
            sites.get(r, i, cx, cy, cz);

            // ---- scan, then sort: lane k owns neighbour k
            int m;
            const bool over = !scan_list(sites, r, i, cx, cy, cz, bc, va.rl2, keys, idx, lane, m);
            const bool mine = !over && lane < m;
            unsigned long long key = ~0ULL;
            int jn = -1;
            if (!over) // wave-uniform
                rank_sort(keys, idx, m, lane, key, jn);

            // lane k < m: neighbour k.  rho^2 from the key (the bits of the signed image's), d the signed image
            const double r2 = mine ? __longlong_as_double((long long)key) : 0.0;
            double ox, oy, oz;
            sites.get(r, mine ? jn : i, ox, oy, oz);
            const double dx = vector1D(cx, ox, bc), dy = vector1D(cy, oy, bc), dz = vector1D(cz, oz, bc);

            int flags = over ? VO_CAP : 0;
            if (!over && (m == 0 || lane_f64(r2, 0) == 0.0)) // no neighbour, or a coincident one: no cell
                flags = VO_OPEN;

            int cnt = 0;         // the vertices of lane k's polygon; 0: no face
            double g2 = 0.0;     // the largest s s + t t of them
            const double h = 0.25 * r2;
            if (flags == 0) { // wave-uniform
                // ---- face k: the basis (u, v) of its plane, the square, the clips in rising rank
                const double fx = fabs(dx), fy = fabs(dy), fz = fabs(dz);
                const int axis = (fx <= fy && fx <= fz) ? 0 : (fy <= fz ? 1 : 2); // the first of equal ones
                const double wx = axis == 0 ? 0.0 : (axis == 1 ? -dz : dy);
                const double wy = axis == 0 ? dz : (axis == 1 ? 0.0 : -dx);
                const double wz = axis == 0 ? -dy : (axis == 1 ? dx : 0.0);
                const double wn = sqrt((wx * wx + wy * wy) + wz * wz);
                const double ux = wx / wn, uy = wy / wn, uz = wz / wn;
                const double qx = dy * uz - dz * uy, qy = dz * ux - dx * uz, qz = dx * uy - dy * ux;
                const double qn = sqrt((qx * qx + qy * qy) + qz * qz);
                const double vx = qx / qn, vy = qy / qn, vz = qz / qn;
                const double mx = 0.5 * dx, my = 0.5 * dy, mz = 0.5 * dz;
                const double rl = va.rl;
                if (mine) {
                    poly[0] = make_double2(-rl, -rl);
                    poly[64] = make_double2(rl, -rl);
                    poly[128] = make_double2(rl, rl);
                    poly[192] = make_double2(-rl, rl);
                    cnt = 4;
                }
                g2 = rl * rl + rl * rl;
                bool stopped = false, bad_face = false;
                for (int pm = 0; pm < m; pm++) {
                    const double r2m = lane_f64(r2, pm);
                    if (va.prune)
                        stopped = stopped || 0.25 * r2m > (h + g2) * prune_margin;
                    const bool left = cnt > 0 && !stopped;
                    if (wave_ballot(left) == 0ULL)
                        break; // no later plane reaches any polygon
                    const bool act = left && lane != pm;
                    const double ex = lane_f64(dx, pm), ey = lane_f64(dy, pm), ez = lane_f64(dz, pm);
                    if (act) {
                        const double a = (ux * ex + uy * ey) + uz * ez, b = (vx * ex + vy * ey) + vz * ez;
                        const double c = 0.5 * r2m - ((mx * ex + my * ey) + mz * ez);
                        // the whole polygon into registers first (independent reads, one wait), then
                        // the pass writes the new list over it
                        double2 vt[MMC_VORONOI_MAXV];
                        double ev[MMC_VORONOI_MAXV];
#pragma unroll
                        for (int j = 0; j < MMC_VORONOI_MAXV; j++)
                            vt[j] = j < cnt ? poly[64 * j] : make_double2(0.0, 0.0);
#pragma unroll
                        for (int j = 0; j < MMC_VORONOI_MAXV; j++)
                            ev[j] = (a * vt[j].x + b * vt[j].y) - c;
                        int o = 0, cuts = 0;
                        double gn = 0.0;
                        bool bad = false;
#pragma unroll
                        for (int j = 0; j < MMC_VORONOI_MAXV; j++) {
                            if (j < cnt && !bad) {
                                const double2 p = vt[j];
                                const double sp = ev[j];
                                const bool wrap = j + 1 >= cnt;
                                const double2 q = wrap ? vt[0] : vt[(j + 1) % MMC_VORONOI_MAXV];
                                const double sq = wrap ? ev[0] : ev[(j + 1) % MMC_VORONOI_MAXV];
                                const bool pin = sp <= 0.0, qin = sq <= 0.0;
                                if (pin) {
                                    if (o >= MMC_VORONOI_MAXV) {
                                        bad = true;
                                    } else {
                                        poly[64 * o] = p;
                                        gn = fmax(gn, p.x * p.x + p.y * p.y);
                                        o++;
                                    }
                                }
                                if (pin != qin && !bad) {
                                    if (++cuts > 2 || o >= MMC_VORONOI_MAXV) {
                                        bad = true;
                                    } else {
                                        const double w = sp / (sp - sq);
                                        const double2 x = make_double2(p.x + w * (q.x - p.x), p.y + w * (q.y - p.y));
                                        poly[64 * o] = x;
                                        gn = fmax(gn, x.x * x.x + x.y * x.y);
                                        o++;
                                    }
                                }
                            }
                        }
                        bad_face = bad_face || bad;
                        cnt = (bad || o < 3) ? 0 : o;
                        g2 = gn;
                    }
                }
                const unsigned long long alive = wave_ballot(cnt > 0);
                const bool open = alive == 0ULL || wave_ballot(cnt > 0 && 4.0 * (h + g2) > va.rl2) != 0ULL;
                flags = (wave_ballot(bad_face) != 0ULL ? VO_POLY : 0) | (open ? VO_OPEN : 0);
            }

            if (flags != 0) { // wave-uniform: in no histogram and no sum
                if (lane < 3 && ((flags >> lane) & 1))
                    atomicAdd(&hw[lane], 1u);
                if (lane == 0) {
                    if (va.vol)
                        va.vol[g] = nan;
                    if (va.area)
                        va.area[g] = nan;
                    if (va.carea)
                        va.carea[g] = 0.0;
                    if (va.faces)
                        va.faces[g] = -flags;
                }
                if (va.nbr)
                    va.nbr[MMC_VORONOI_CAP * g + lane] = -1;
                if (va.face_area)
                    va.face_area[MMC_VORONOI_CAP * g + lane] = 0.0;
                continue;
            }

            // ---- the areas, then the cell's sums in rising rank (a lane without a face adds 0.0)
            double A = 0.0;
            if (cnt > 0) {
                double2 p = poly[0];
                const double2 first = p;
                double acc = 0.0;
                for (int j = 0; j < cnt; j++) {
                    const double2 q = j + 1 < cnt ? poly[64 * (j + 1)] : first;
                    acc = acc + (p.x * q.y - q.x * p.y);
                    p = q;
                }
                A = 0.5 * fabs(acc);
            }
            const double rho = sqrt(r2);
            const bool counted = A > va.area_min;
            const double Ar = A * rho, Ac = counted ? A : 0.0;
            double S = 0.0, T = 0.0, C = 0.0;
            for (int k = 0; k < m; k++) {
                S = S + lane_f64(A, k);
                T = T + lane_f64(Ar, k);
                C = C + lane_f64(Ac, k);
            }
            const double V = T / 6.0;
            const double eta = ((S * S) * S) / ((va.k36pi * V) * V);
            const unsigned long long cm = wave_ballot(counted);
            const int nf = __popcll(cm);

            if (lane == 0) {
                if (va.vol_hist)
                    atomicAdd(&hw[3 + vo_bin(V * va.v_scale, va.v_bins)], 1u);
                if (va.eta_hist)
                    atomicAdd(&hw[va.o_eta + vo_bin((eta - 1.0) * va.eta_scale, va.eta_bins)], 1u);
                if (va.face_hist)
                    atomicAdd(&hw[va.o_face + nf], 1u);
                if (va.vol)
                    va.vol[g] = V;
                if (va.area)
                    va.area[g] = S;
                if (va.carea)
                    va.carea[g] = C;
                if (va.faces)
                    va.faces[g] = nf;
            }
            if (counted) {
                if (va.side_hist)
                    atomicAdd(&hw[va.o_side + cnt], 1u); // 3 .. MMC_VORONOI_MAXV
                if (va.nbr_hist)
                    atomicAdd(&hw[va.o_nbr + vo_bin(rho * va.inv_dr, va.r_bins)], 1u);
            }
            // counted faces in rising rank, then -1 and 0
            const int slot = lanes_below(cm);
            if (va.nbr) {
                if (counted)
                    va.nbr[MMC_VORONOI_CAP * g + slot] = jn;
                if (lane >= nf)
                    va.nbr[MMC_VORONOI_CAP * g + lane] = -1;
            }
            if (va.face_area) {
                if (counted)
                    va.face_area[MMC_VORONOI_CAP * g + slot] = A;
                if (lane >= nf)
                    va.face_area[MMC_VORONOI_CAP * g + lane] = 0.0;
            }
        }

        // the workgroup's counters added to the replica's (or the summed) ones and cleared, once every
        // wave has left the replica (the waves of a workgroup walk the same replicas: the barriers match)
        __syncthreads();
        const int64_t ro = va.per_replica ? r : 0;
        for (int q = tid; q < hs; q += (int)blockDim.x) {
            const unsigned v = hw[q];
            if (v != 0u) {
                unsigned long long *dst;
                if (q < 3)
                    dst = va.flagged + 3 * (int64_t)r + q;
                else if (q < va.o_eta)
                    dst = va.vol_hist + ro * (va.v_bins + 1) + (q - 3);
                else if (q < va.o_face)
                    dst = va.eta_hist + ro * (va.eta_bins + 1) + (q - va.o_eta);
                else if (q < va.o_side)
                    dst = va.face_hist + ro * (MMC_VORONOI_CAP + 1) + (q - va.o_face);
                else if (q < va.o_nbr)
                    dst = va.side_hist + ro * (MMC_VORONOI_MAXV + 1) + (q - va.o_side);
                else
                    dst = va.nbr_hist + ro * (va.r_bins + 1) + (q - va.o_nbr);
                atomicAdd(dst, (unsigned long long)v);
                hw[q] = 0u;
            }
        }
        if constexpr (!STAGE)
            __syncthreads(); // (STAGE: the barrier before the next replica's copy)
    }
}

// One wave per replica, k_local_qsum's order: lane l adds the terms of the unflagged molecules
// i = l, l + 64, ... in that order, then the 64 lane sums are added by wave_sum_rows.
// out[r][8] = (number summed, sum V, sum V V, sum S, sum eta, sum counted faces, sum counted area, 0).
__global__ __launch_bounds__(NBR_WAVES * 64) void k_voronoi_sums(const double *__restrict__ vol, const double *__restrict__ area,
                                                                const double *__restrict__ carea,
                                                                const int32_t *__restrict__ faces, double k36pi,
                                                                double *out, int n_mol, int R)
{
    const int lane = threadIdx.x & 63;
    const int r = (int)blockIdx.x * NBR_WAVES + (int)(threadIdx.x >> 6);
    if (r >= R)
        return;
    double a[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    int cnt = 0;
    for (int i = lane; i < n_mol; i += 64) {
        const int64_t g = (int64_t)r * n_mol + i;
        const int f = faces[g];
        if (f >= 0) {
            const double V = vol[g], S = area[g];
            a[0] += V;
            a[1] += V * V;
            a[2] += S;
            a[3] += ((S * S) * S) / ((k36pi * V) * V);
            a[4] += (double)f;
            a[5] += carea[g];
            cnt++;
        }
    }
    double s[6];
#pragma unroll
    for (int q = 0; q < 6; q++)
        s[q] = wave_sum_rows(a[q]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        cnt += __shfl_xor(cnt, off, 64);
    if (lane == 0) {
        double *o = out + 8 * (int64_t)r;
        o[0] = (double)cnt;
#pragma unroll
        for (int q = 0; q < 6; q++)
            o[1 + q] = s[q];
        o[7] = 0.0;
    }
}
