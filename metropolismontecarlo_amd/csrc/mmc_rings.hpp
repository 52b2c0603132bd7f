// mmc_rings.hpp -- the shortest-path rings of every replica's hydrogen-bond graph, read-only beside the
// chains:
//   k_hbond_rings   per replica: the bonds of every molecule with their box vectors and donations, then
//                   every ring of 3 .. n_max molecules without a shortcut, by size: wrapping or not,
//                   homodromic or not, and per molecule
// The definitions are stated in include/mmc_hip.h ("Hydrogen-bond rings") and restated in numpy by
// tests/rings_ref.py.  The graph is k_hbond_network's for one criterion; this kernel carries its own
// copy of mmc_nbr.hpp's staging, scan (scan_candidates) and bond test (HbPair), which also keeps the two
// donation bits: on the shared helpers its ring search, untouched, compiled to code that ran 0.5 to
// 0.9 % slower at n_max = 6 and 8 (profiles/nbr_scaffold_bench.json), so the copy stays.  A change to
// either is to be made in both.
//
// One persistent workgroup per replica, whole replicas in turn.  One replica:
//   stage    the O positions into LDS, as k_hbond_network.
//   bonds    k_hbond_network's scan for one criterion.  A list holds MMC_RING_MAX_DEG entries of 32
//            bits (entry e of all molecules side by side): j in bits 0..10, the box vector m_ij in
//            11..15 (base 3), bit 16 "i donates to j", bit 17 "j donates to i"; the degree is counted
//            beyond the list (it flags the replica) in one byte, saturating.
//   rings    a wave per lowest member v.  In a shortest-path ring of n members the k-th member lies at
//            graph distance min(k, n - k) from v: both halves of the ring are geodesics from v.  So the
//            wave first writes the breadth-first levels from v, truncated at n_max / 2, into its own
//            byte array in LDS (one sweep over the molecules per level; a sweep reads only levels of
//            the sweep before).  Then lane (a, s) -- a a partner of v above v that is not v's largest,
//            s a slot of a's list -- walks depth-first every path v, a, (a's s-th partner), ... whose
//            levels rise by one per step to a peak, stay once (odd n) or not (even n), and fall by one
//            per step back to level 1, through members above v that differ from the rising member of
//            their level, and that ends at a partner of v above a: every candidate once, in canonical
//            direction.  The stack is one 4-bit slot index per depth in one register, the path eight
//            16-bit members in two 64-bit registers.  A candidate is then tested pair by pair among
//            its members other than v (whose distances are the levels): ring distance 2 means not
//            bonded, 3 means no common partner either, 4 also no partner of the one bonded to a partner
//            of the other -- all through the lists, at most 8, 64 and 512 comparisons.  With at most 8
//            entries per list every loop has a fixed bound (DESIGN.md has the worst case).
//   sums     LDS integer adds: the three rows by size, six counts per molecule (in the space of the
//            positions), the rows claimed in ring_out; then per molecule the membership bins, and one
//            thread writes the stats.  No floating point after the bonds.
// Everything is an integer and every accumulation an integer add or max: no order of lanes, waves or
// workgroups can change a bit, except which row of ring_out a ring lands in.
#pragma once
#include "mmc_network.hpp"

#define RG_THREADS 1024       // the largest workgroup (the host launches 4, 8 or 16 waves)
#define RG_NONE 0xFFu         // the level of a molecule farther than n_max / 2 from v
#define RG_R_HIST 0           // [3][9] rings by size
#define RG_R_MEMBER 27        // [9][33] molecules by membership
#define RG_R_FLAG 324
#define RG_R_TWICE 325        // the sum of the degrees
#define RG_R_NORING 326
#define RG_R_MOST 327
#define RG_R_ROWS 328         // row-0 rings so far: the next row of ring_out
#define RG_R_DROPPED 329
#define RG_RED 336
static_assert(MMC_RING_MAX_SIZE == 8 && MMC_RING_MAX_DEG == 8 && MMC_RING_STATS == 8 && MMC_RING_MEMBER_BINS == 33 &&
                  MMC_NET_MAX_MOL <= 2048,
              "a path is eight members of 16 bits, a stack seven slots of 4 bits, a list entry 11 bits of j");
static_assert(RG_R_MEMBER == 3 * (MMC_RING_MAX_SIZE + 1) && RG_R_FLAG == RG_R_MEMBER + (MMC_RING_MAX_SIZE + 1) * MMC_RING_MEMBER_BINS,
              "the rows of the LDS sums follow one another");

struct RingArgs {
    const double *box_r;             // [R] per-replica boxes, or NULL: bv.box
    unsigned long long *ring_hist;   // [3][9] or [R][3][9], zeroed by the host; or NULL
    unsigned long long *member_hist; // [9][33] or [R][9][33], zeroed by the host; or NULL
    long long *stats;                // [R][8]
    unsigned short *count;           // [nr][N][9] of this launch's replicas, or NULL
    int32_t *ring;                   // [nr][max_rings][8] of this launch's replicas, filled with -1; or NULL
    long long max_rings;
    double rhb2, cos2;
    int32_t n_max, per_replica;
    int32_t r0, nr;                  // the replicas of this launch
};

// dynamic LDS of a workgroup of nw waves: offsets of the regions
struct RingLds {
    size_t adj, deg, lev, cand, red, bytes;
    int lev_stride;
};
__host__ __device__ inline RingLds ring_lds(int n_mol, int nw)
{
    auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
    RingLds l;
    l.adj = up(24 * (size_t)n_mol);                                   // positions [3][N], then counts [6][N]
    l.deg = l.adj + 4 * (size_t)MMC_RING_MAX_DEG * n_mol;             // lists [8][N] of 32 bits
    l.lev = up(l.deg + (size_t)n_mol);                                // degrees [N] of 8 bits
    l.lev_stride = (int)up((size_t)n_mol);
    l.cand = l.lev + (size_t)nw * l.lev_stride;                       // levels [nw][N] of 8 bits
    l.red = l.cand + 4 * (size_t)nw * NBR_CAND;
    l.bytes = l.red + 4 * RG_RED;
    return l;
}

// the members of a path: eight of 16 bits in two words
struct RingPath {
    unsigned long long lo, hi;
    __device__ __forceinline__ int get(int k) const { return (int)(((k < 4 ? lo : hi) >> (16 * (k & 3))) & 0xFFFFull); }
    __device__ __forceinline__ void set(int k, int v)
    {
        const unsigned long long m = 0xFFFFull << (16 * (k & 3)), w = (unsigned long long)v << (16 * (k & 3));
        if (k < 4)
            lo = (lo & ~m) | w;
        else
            hi = (hi & ~m) | w;
    }
};

// is there a path of at most `dmax` (1, 2 or 3) bonds between x and y?  Through the lists alone.
__device__ __forceinline__ bool ring_within(const unsigned *__restrict__ adj, const unsigned char *__restrict__ degc, int n_mol,
                                            int x, int y, int dmax)
{
    const int dx = degc[x], dy = degc[y];
    for (int s = 0; s < dx; s++)
        if ((int)(adj[s * n_mol + x] & 2047u) == y)
            return true;
    if (dmax < 2)
        return false;
    for (int s = 0; s < dx; s++) {
        const int z = (int)(adj[s * n_mol + x] & 2047u);
        for (int t = 0; t < dy; t++)
            if ((int)(adj[t * n_mol + y] & 2047u) == z)
                return true;
    }
    if (dmax < 3)
        return false;
    for (int s = 0; s < dx; s++) {
        const int z = (int)(adj[s * n_mol + x] & 2047u), dz = degc[z];
        for (int t = 0; t < dy; t++) {
            const int w = (int)(adj[t * n_mol + y] & 2047u);
            for (int u = 0; u < dz; u++)
                if ((int)(adj[u * n_mol + z] & 2047u) == w)
                    return true;
        }
    }
    return false;
}

// REC: molecules are the 128-byte records of homogeneous batches; else the SoA arrays (load_sites9).
// grid: any number of workgroups of 4, 8 or 16 waves; workgroup g of G takes the replicas r0 + g,
// r0 + g + G, ... of the launch.
template <bool REC>
__global__ __launch_bounds__(RG_THREADS) void k_hbond_rings(BatchView bv, const double *__restrict__ rec, RingArgs ra)
{
    extern __shared__ __align__(16) unsigned char rg_lds[];
    const int tid = threadIdx.x, lane = tid & 63, nt = (int)blockDim.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nw = nt >> 6;
    const int n_mol = bv.n_mol, n_max = ra.n_max;
    const RingLds lo = ring_lds(n_mol, nw);
    double *const pos = reinterpret_cast<double *>(rg_lds);
    unsigned *const cnt = reinterpret_cast<unsigned *>(rg_lds);
    unsigned *const adj = reinterpret_cast<unsigned *>(rg_lds + lo.adj);
    unsigned char *const degc = rg_lds + lo.deg;
    unsigned char *const lev = rg_lds + lo.lev + (size_t)wv * lo.lev_stride;
    int *const cand = reinterpret_cast<int *>(rg_lds + lo.cand) + wv * NBR_CAND;
    unsigned *const red = reinterpret_cast<unsigned *>(rg_lds + lo.red);

    for (int rl = (int)blockIdx.x; rl < ra.nr; rl += (int)gridDim.x) {
        const int r = ra.r0 + rl;
        const BoxConsts bc = box_consts(ra.box_r ? ra.box_r[r] : bv.box);
        const int64_t ro = ra.per_replica ? r : 0;
        long long *const st = ra.stats + (int64_t)r * MMC_RING_STATS;
        unsigned short *const cnt_out = ra.count ? ra.count + (int64_t)rl * n_mol * (MMC_RING_MAX_SIZE + 1) : nullptr;
        int32_t *const ring_out = ra.ring ? ra.ring + (int64_t)rl * ra.max_rings * MMC_RING_MAX_SIZE : nullptr;

        __syncthreads(); // every thread has left the counts of the replica before
        for (int j = tid; j < n_mol; j += nt) {
            double x, y, z;
            if constexpr (REC) {
                const double *p = rec + ((int64_t)r * n_mol + j) * MMC_RSTRIDE;
                const double2 v0 = *reinterpret_cast<const double2 *>(p);
                x = v0.x; y = v0.y; z = p[2];
            } else {
                const int64_t a0 = (int64_t)r * bv.atom_stride + bv.first0[j];
                x = bv.ax[a0]; y = bv.ay[a0]; z = bv.az[a0];
            }
            pos[j] = x; pos[n_mol + j] = y; pos[2 * n_mol + j] = z;
        }
        for (int q = tid; q < RG_RED; q += nt)
            red[q] = 0u;
        __syncthreads();

        // ---- bonds: a wave per molecule i (k_hbond_network's scan, one criterion, donations kept) ----
        for (int i = wv; i < n_mol; i += nw) {
            double ci[9]; // the wave's molecule: wave-uniform
            load_sites9<REC>(bv, rec, r, i, ci);
            double ui[2][3]; // d(O_i, H_i,h)
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int d = 0; d < 3; d++)
                    ui[h][d] = vector1D(ci[d], ci[3 + 3 * h + d], bc);
            int dg = 0, n_cand = 0; // wave-uniform

            // candidates [0, n) of the list, one per lane (n <= 64), in ascending j
            auto bonds = [&](int n) {
                bool b = false;
                unsigned entry = 0u;
                if (lane < n) {
                    const int j = cand[lane];
                    double cj[9];
                    load_sites9<REC>(bv, rec, r, j, cj);
                    const double vx = vector1D(ci[0], cj[0], bc), vy = vector1D(ci[1], cj[1], bc),
                                 vz = vector1D(ci[2], cj[2], bc);
                    const double vv = (vx * vx + vy * vy) + vz * vz;
                    const double wx = vector1D(cj[0], ci[0], bc), wy = vector1D(cj[1], ci[1], bc),
                                 wz = vector1D(cj[2], ci[2], bc);
                    const double ww = (wx * wx + wy * wy) + wz * wz;
                    // the boxes vector1D added to O_j - O_i, per component, + 1
                    unsigned code = 0u;
#pragma unroll
                    for (int d = 2; d >= 0; d--) {
                        const double dd = cj[d] - ci[d];
                        const unsigned m1 = fabs(dd) < bc.half ? 1u : (dd > 0.0 ? 0u : 2u);
                        code = 3u * code + m1;
                    }
                    bool don[2] = { false, false }; // i donates to j; j donates to i
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        const double t0 = (ui[h][0] * vx + ui[h][1] * vy) + ui[h][2] * vz;
                        const double q0 = ((ui[h][0] * ui[h][0] + ui[h][1] * ui[h][1]) + ui[h][2] * ui[h][2]) * vv;
                        const double ux = vector1D(cj[0], cj[3 + 3 * h], bc), uy = vector1D(cj[1], cj[4 + 3 * h], bc),
                                     uz = vector1D(cj[2], cj[5 + 3 * h], bc);
                        const double t1 = (ux * wx + uy * wy) + uz * wz;
                        const double q1 = ((ux * ux + uy * uy) + uz * uz) * ww;
                        don[0] = don[0] || (t0 > 0.0 && t0 * t0 >= ra.cos2 * q0); // HbPair::bonded
                        don[1] = don[1] || (t1 > 0.0 && t1 * t1 >= ra.cos2 * q1);
                    }
                    const bool in = vv < ra.rhb2;
                    don[0] = don[0] && in;
                    don[1] = don[1] && in;
                    b = don[0] || don[1];
                    entry = (unsigned)j | (code << 11) | (don[0] ? 1u << 16 : 0u) | (don[1] ? 1u << 17 : 0u);
                }
                const unsigned long long m = wave_ballot(b);
                const int slot = dg + lanes_below(m);
                if (b && slot < MMC_RING_MAX_DEG)
                    adj[slot * n_mol + i] = entry;
                dg += __popcll(m);
            };

            for (int jb = 0; jb < n_mol; jb += 64) {
                const int j = jb + lane;
                const bool valid = j < n_mol && j != i;
                const int jj = min(j, n_mol - 1);
                const double dx = vector1D_abs(ci[0], pos[jj], bc), dy = vector1D_abs(ci[1], pos[n_mol + jj], bc),
                             dz = vector1D_abs(ci[2], pos[2 * n_mol + jj], bc);
                const double r2 = (dx * dx + dy * dy) + dz * dz;
                const bool near = valid && r2 < ra.rhb2;
                const unsigned long long nm = wave_ballot(near);
                if (nm != 0ULL) { // wave-uniform
                    if (near)
                        cand[n_cand + lanes_below(nm)] = j; // n_cand <= 63 here: the slot is < NBR_CAND
                    n_cand += __popcll(nm);
                    wave_sync();
                    if (n_cand >= 64) {
                        bonds(64);
                        const int rest = n_cand - 64; // <= 63: one lane each
                        const int mv = lane < rest ? cand[64 + lane] : 0;
                        wave_sync();
                        if (lane < rest)
                            cand[lane] = mv;
                        wave_sync();
                        n_cand = rest;
                    }
                }
            }
            if (n_cand > 0)
                bonds(n_cand);
            wave_sync(); // the candidate list is rewritten by the wave's next molecule
            if (lane == 0)
                degc[i] = (unsigned char)min(dg, 255);
        }
        __syncthreads(); // the lists are complete, the positions no longer read

        for (int i = tid; i < n_mol; i += nt) {
            const unsigned d = degc[i];
            if (d > MMC_RING_MAX_DEG)
                red[RG_R_FLAG] = 1u;
            else
                atomicAdd(&red[RG_R_TWICE], d);
        }
        for (int q = tid; q < 6 * n_mol; q += nt)
            cnt[q] = 0u;
        __syncthreads();
        if (red[RG_R_FLAG] != 0u) { // workgroup-uniform: the defined values, no histogram
            if (tid < MMC_RING_STATS)
                st[tid] = tid == 7 ? 1 : 0;
            if (cnt_out)
                for (int q = tid; q < n_mol * (MMC_RING_MAX_SIZE + 1); q += nt)
                    cnt_out[q] = 0xFFFFu;
            continue; // (the rows of ring_out are -1 already)
        }

        // ---- rings: a wave per lowest member v ---------------------------------------------------------
        const int n_half = n_max >> 1;
        for (int v = wv; v < n_mol; v += nw) {
            const int dv = degc[v];
            const unsigned mine = lane < dv ? adj[lane * n_mol + v] : 0u;
            // the lists ascend: the partners above v are the last n_up entries
            const int n_up = __popcll(wave_ballot(lane < dv && (int)(mine & 2047u) > v));
            if (n_up < 2)
                continue; // wave-uniform: v is the lowest member of no ring
            const int first_up = dv - n_up;

            wave_sync(); // the lanes are done with the levels of the v before
            for (int j = lane; j < n_mol; j += 64)
                lev[j] = RG_NONE;
            wave_sync();
            if (lane < dv)
                lev[mine & 2047u] = 1;
            if (lane == 0)
                lev[v] = 0;
            wave_sync();
            for (int d = 2; d <= n_half; d++) {
                bool any = false;
                for (int j = lane; j < n_mol; j += 64) {
                    if (lev[j] != RG_NONE)
                        continue;
                    const int dj = degc[j];
                    bool hit = false;
                    for (int e = 0; e < dj; e++)
                        hit = hit || lev[adj[e * n_mol + j] & 2047u] == d - 1;
                    if (hit) {
                        lev[j] = (unsigned char)d; // (read by others only as "not d - 1", before and after)
                        any = true;
                    }
                }
                wave_sync();
                if (!wave_any(any))
                    break;
            }

            // lane (ai, s2): a = the ai-th partner above v, not the last; s2 the first step's slot
            const int ai = lane >> 3, s2 = lane & 7;
            if (ai < n_up - 1) {
                const int a = (int)(adj[(first_up + ai) * n_mol + v] & 2047u);
                if (s2 < (int)degc[a]) {
                    RingPath p;
                    p.lo = (unsigned long long)v | ((unsigned long long)a << 16);
                    p.hi = 0ULL;
                    unsigned stk = (unsigned)s2 << 4; // depth k's next slot in bits 4 k .. 4 k + 3
                    int k = 1, peak = 0;              // peak: the depth of the first member that does not rise
                    while (k >= 1) {
                        const int x = p.get(k);
                        const int s = (int)((stk >> (4 * k)) & 15u);
                        if (k == 1 && s > s2)
                            break; // this lane's slot of a is worked off
                        if (s >= (int)degc[x]) {
                            stk &= ~(15u << (4 * k));
                            k--;
                            if (peak > k)
                                peak = 0;
                            continue;
                        }
                        stk += 1u << (4 * k);
                        const int y = (int)(adj[s * n_mol + x] & 2047u);
                        if (y <= v)
                            continue;
                        const int lx = lev[x], ly = lev[y];
                        if (peak == 0) {
                            if (ly == lx + 1 && 2 * ly <= n_max) { // rising (ly <= n_half: never RG_NONE)
                                k++;
                                p.set(k, y);
                                continue;
                            }
                            if (!((ly == lx && 2 * lx + 1 <= n_max) || (ly == lx - 1 && lx >= 2)))
                                continue;
                        } else if (ly != lx - 1) {
                            continue;
                        }
                        if (ly < lx && y == p.get(ly))
                            continue; // the rising member of that level
                        if (ly != 1) { // falling on
                            if (peak == 0)
                                peak = k + 1;
                            k++;
                            p.set(k, y);
                            continue;
                        }
                        if (y <= a)
                            continue;

                        // a candidate of n members: p[0 .. k], y
                        const int n = k + 2;
                        RingPath c = p;
                        c.set(k + 1, y);
                        bool ok = true;
                        for (int i = 1; i < n - 1 && ok; i++)
                            for (int j = i + 2; j < n && ok; j++) {
                                const int dr = min(j - i, n - (j - i));
                                ok = !ring_within(adj, degc, n_mol, c.get(i), c.get(j), dr - 1);
                            }
                        if (!ok)
                            continue;
                        int mx = 0, my = 0, mz = 0;
                        unsigned both = 3u;
                        for (int i = 0; i < n; i++) {
                            const int xi = c.get(i), yi = c.get(i + 1 == n ? 0 : i + 1), di = degc[xi];
                            unsigned en = 0u;
                            for (int e = 0; e < di; e++) {
                                const unsigned ee = adj[e * n_mol + xi];
                                if ((int)(ee & 2047u) == yi)
                                    en = ee;
                            }
                            const int cd = (int)((en >> 11) & 31u);
                            mx += cd % 3 - 1;
                            my += cd / 3 % 3 - 1;
                            mz += cd / 9 - 1;
                            both &= en >> 16;
                        }
                        if ((mx | my | mz) != 0) {
                            atomicAdd(&red[RG_R_HIST + (MMC_RING_MAX_SIZE + 1) + n], 1u);
                            continue;
                        }
                        atomicAdd(&red[RG_R_HIST + n], 1u);
                        if (both != 0u)
                            atomicAdd(&red[RG_R_HIST + 2 * (MMC_RING_MAX_SIZE + 1) + n], 1u);
                        for (int i = 0; i < n; i++)
                            atomicAdd(&cnt[(n - 3) * n_mol + c.get(i)], 1u);
                        const unsigned row = atomicAdd(&red[RG_R_ROWS], 1u);
                        if (ring_out) {
                            if ((long long)row < ra.max_rings) {
                                int32_t *const o = ring_out + (int64_t)row * MMC_RING_MAX_SIZE;
                                for (int i = 0; i < MMC_RING_MAX_SIZE; i++)
                                    o[i] = i < n ? c.get(i) : -1;
                            } else {
                                atomicAdd(&red[RG_R_DROPPED], 1u);
                            }
                        }
                    }
                }
            }
        }
        __syncthreads(); // every ring is counted

        // ---- sums: per molecule, then per replica -------------------------------------------------------
        for (int i = tid; i < n_mol; i += nt) {
            unsigned tot = 0u;
            for (int n = 3; n <= MMC_RING_MAX_SIZE; n++) {
                const unsigned c = cnt[(n - 3) * n_mol + i];
                tot += c;
                if (n <= n_max)
                    atomicAdd(&red[RG_R_MEMBER + n * MMC_RING_MEMBER_BINS + min(c, (unsigned)(MMC_RING_MEMBER_BINS - 1))], 1u);
                if (cnt_out)
                    cnt_out[i * (MMC_RING_MAX_SIZE + 1) + n] = (unsigned short)min(c, 65535u);
            }
            atomicAdd(&red[RG_R_MEMBER + min(tot, (unsigned)(MMC_RING_MEMBER_BINS - 1))], 1u);
            if (tot == 0u)
                atomicAdd(&red[RG_R_NORING], 1u);
            atomicMax(&red[RG_R_MOST], tot);
            if (cnt_out) {
                cnt_out[i * (MMC_RING_MAX_SIZE + 1)] = (unsigned short)min(tot, 65535u);
                cnt_out[i * (MMC_RING_MAX_SIZE + 1) + 1] = 0;
                cnt_out[i * (MMC_RING_MAX_SIZE + 1) + 2] = 0;
            }
        }
        __syncthreads();
        if (tid == 0) {
            unsigned rows[3] = { 0u, 0u, 0u };
            for (int q = 0; q < 3; q++)
                for (int n = 3; n <= MMC_RING_MAX_SIZE; n++)
                    rows[q] += red[RG_R_HIST + q * (MMC_RING_MAX_SIZE + 1) + n];
            st[0] = red[RG_R_TWICE] / 2u;
            st[1] = rows[0];
            st[2] = rows[1];
            st[3] = rows[2];
            st[4] = red[RG_R_NORING];
            st[5] = red[RG_R_MOST];
            st[6] = red[RG_R_DROPPED];
            st[7] = 0;
        }
        if (ra.ring_hist)
            for (int q = tid; q < RG_R_MEMBER; q += nt)
                if (red[RG_R_HIST + q] != 0u)
                    atomicAdd(ra.ring_hist + ro * RG_R_MEMBER + q, (unsigned long long)red[RG_R_HIST + q]);
        if (ra.member_hist)
            for (int q = tid; q < RG_R_FLAG - RG_R_MEMBER; q += nt)
                if (red[RG_R_MEMBER + q] != 0u)
                    atomicAdd(ra.member_hist + ro * (RG_R_FLAG - RG_R_MEMBER) + q, (unsigned long long)red[RG_R_MEMBER + q]);
    }
}
