// mmc_network.hpp -- the hydrogen-bond network of every replica, read-only beside the chains:
//   k_hbond_network   per (replica, criterion): the bonds of every molecule, the connected components
//                     of the bond graph on the selected sites, their sizes and the axes along which
//                     they wrap the periodic box
// The definitions are stated in include/mmc_hip.h ("Hydrogen-bond network") and restated in numpy by
// tests/network_ref.py; staging, scan and bond test are mmc_nbr.hpp's
// (stage_sites, scan_candidates, HbPair).
//
// One persistent workgroup per replica, whole replicas in turn.  The criteria of a call are worked
// off in groups of `group`: as many as have their adjacency lists in the workgroup's LDS at once.
// One group, one replica:
//   stage    the replica's O positions into LDS (stage_sites).
//   bonds    every wave takes molecules i = wave, wave + nw, ...; lane l scans j = l, l + 64, ... and
//            lanes with r^2 < max r_hb^2 of the group append j to the wave's candidate list (ballot +
//            prefix count), worked off 64 at a time in ascending j: lane n loads candidate n's sites,
//            tests both directions through both hydrogens per criterion, and the bonded lanes of a
//            criterion append (j, boxes) to i's list of that criterion -- again ballot + prefix
//            count, so the list is in ascending j.  A list holds MMC_NET_MAX_DEG entries of 16 bits
//            (entry e of all molecules side by side: consecutive lanes read consecutive words):
//            j in 11 and the box vector m_ij in 5 (base 3); the degree is counted beyond that (it
//            flags the replica) in one byte, saturating.
//   clusters per criterion, all threads.  Every site starts with its own index as label and offset
//            (0, 0, 0), packed into 64 bits: label << 48 | three offsets biased by 0x8000.  A round
//            reads one buffer and writes the other: a site takes the smallest word among its own and
//            (label_j, offset_j - m_ij) of the neighbours with a SMALLER label.  One workgroup barrier
//            per round; the rounds end when one changed nothing (a flag in LDS, three in rotation so
//            that none is cleared while it may still be read).  The label 0 .. N - 1 travels one bond
//            per round: the number of rounds is the largest bond distance of a site from the lowest
//            index of its cluster, plus one.
//            At the fixed point every non-root site took its word from a neighbour that already had
//            its final one: the offsets are the potential of a spanning tree.  An edge (i, j) with
//            offset_i + m_ij != offset_j closes a walk that winds: its nonzero components are OR-ed
//            into the cluster's mask (LDS atomics by root; any order).  Sizes by root likewise, then
//            the roots add to the size histogram of the replica in LDS and to the seven sums.
// Everything is an integer and every accumulation an integer add, or, max: no order of lanes, waves
// or workgroups can change a bit.  Global atomics: the nonzero bins of the two histograms, once per
// (replica, criterion).
#pragma once
#include "mmc_nbr.hpp"

#define NET_THREADS 1024        // the largest workgroup (the host launches 4, 8 or 16 waves)
#define NET_NONE 0xFFFFu        // the label of a molecule that is no site
#define NET_RED 32              // [0..16] molecules by degree, then NET_R_*
#define NET_R_FLAG 17
#define NET_R_SITES 19
#define NET_R_CLUSTERS 20
#define NET_R_LARGEST 21
#define NET_R_S2 22
#define NET_R_MASK 23
#define NET_R_WRAPPING 24
#define NET_R_CHANGED 25        // .. 27
static_assert(MMC_NET_MAX_MOL <= 2048 && MMC_NET_MAX_DEG == 16 && MMC_NET_MAX_CRIT == 8 && MMC_NET_STATS == 8,
              "a list entry is 11 bits of j and 5 of boxes; N^2 (the sum of s^2) stays in 32 bits");

struct NetArgs {
    const double *box_r;             // [R] per-replica boxes, or NULL: bv.box
    unsigned long long *size_hist;   // [K][N + 1] or [R][K][N + 1], zeroed by the host; or NULL
    unsigned long long *deg_hist;    // [K][17] or [R][K][17], zeroed by the host; or NULL
    long long *stats;                // [R][K][8]
    int32_t *label;                  // [R][K][N] or NULL
    int32_t *nbr;                    // [R][K][N][16] or NULL
    double rhb2[MMC_NET_MAX_CRIT], cos2[MMC_NET_MAX_CRIT];
    int32_t min_bonds[MMC_NET_MAX_CRIT];
    int32_t n_crit, group;           // criteria of the call, and of one pass over the molecules
    int32_t per_replica, R;
};

// dynamic LDS of a workgroup of nw waves with `group` criteria per pass: offsets of the regions
struct NetLds {
    size_t adj, deg, hist, cand, red, bytes;
};
__host__ __device__ inline NetLds net_lds(int n_mol, int group, int nw)
{
    auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
    NetLds l;
    l.adj = up(24 * (size_t)n_mol);                                  // positions [3][N], then labels [2][N]
    l.deg = l.adj + 2 * (size_t)MMC_NET_MAX_DEG * group * n_mol;     // lists [group][16][N] of 16 bits
    l.hist = up(l.deg + (size_t)group * n_mol);                      // degrees [group][N] of 8 bits
    l.cand = up(l.hist + 4 * ((size_t)n_mol + 1));                   // clusters by size [N + 1]
    l.red = l.cand + 4 * (size_t)nw * NBR_CAND;
    l.bytes = l.red + 4 * NET_RED;
    return l;
}

// REC: molecules are the 128-byte records of homogeneous batches; else the SoA arrays (load_sites9).
// grid: any number of workgroups of 4, 8 or 16 waves; workgroup g of G takes the replicas g, g + G, ...
template <bool REC>
__global__ __launch_bounds__(NET_THREADS) void k_hbond_network(BatchView bv, const double *__restrict__ rec, NetArgs na)
{
    extern __shared__ __align__(16) unsigned char nt_lds[];
    const int tid = threadIdx.x, lane = tid & 63, nt = (int)blockDim.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nw = nt >> 6;
    const int n_mol = bv.n_mol, K = na.n_crit, G = na.group;
    const NetLds lo = net_lds(n_mol, G, nw);
    double *const pos = reinterpret_cast<double *>(nt_lds);
    unsigned long long *const lab = reinterpret_cast<unsigned long long *>(nt_lds);
    unsigned short *const adj = reinterpret_cast<unsigned short *>(nt_lds + lo.adj);
    unsigned char *const degc = nt_lds + lo.deg;
    unsigned *const shist = reinterpret_cast<unsigned *>(nt_lds + lo.hist);
    int *const cand = reinterpret_cast<int *>(nt_lds + lo.cand) + wv * NBR_CAND;
    unsigned *const red = reinterpret_cast<unsigned *>(nt_lds + lo.red);

    const Sites<REC, true> sites{ bv, rec, pos };

    for (int r = (int)blockIdx.x; r < na.R; r += (int)gridDim.x) {
        const BoxConsts bc = box_consts(na.box_r ? na.box_r[r] : bv.box);
        const int64_t ro = na.per_replica ? r : 0;

        for (int k0 = 0; k0 < K; k0 += G) {
            const int g = min(G, K - k0);
            double rmax2 = 0.0;
            for (int k = 0; k < g; k++)
                rmax2 = fmax(rmax2, na.rhb2[k0 + k]);

            stage_sites(sites, r); // (its first barrier: every thread has left the labels of the pass before)

            // ---- bonds: a wave per molecule i ------------------------------------------------------
            for (int i = wv; i < n_mol; i += nw) {
                double ci[9]; // the wave's molecule: wave-uniform
                load_sites9<REC>(bv, rec, r, i, ci);
                double ui[2][3]; // d(O_i, H_i,h)
                hb_arms(ci, bc, ui);
                int dg[MMC_NET_MAX_CRIT]; // the degrees so far: wave-uniform
#pragma unroll
                for (int k = 0; k < MMC_NET_MAX_CRIT; k++)
                    dg[k] = 0;

                // candidates [0, n) of the list, one per lane (n <= 64), in ascending j
                auto bonds = [&](int n) {
                    unsigned bm = 0u, entry = 0u;
                    if (lane < n) {
                        const int j = cand[lane];
                        double cj[9];
                        load_sites9<REC>(bv, rec, r, j, cj);
                        const HbPair hp(ci, ui, cj, bc);
                        entry = (unsigned)j | (hp.code << 11);
#pragma unroll
                        for (int k = 0; k < MMC_NET_MAX_CRIT; k++)
                            if (k < g) { // criterion k0 + k: any of the four hydrogens, inside its own radius
                                const double c2 = na.cos2[k0 + k];
                                bool b = false;
#pragma unroll
                                for (int h = 0; h < 4; h++)
                                    b = b || hp.bonded(h, c2);
                                if (b && hp.vv < na.rhb2[k0 + k])
                                    bm |= 1u << k;
                            }
                    }
#pragma unroll
                    for (int k = 0; k < MMC_NET_MAX_CRIT; k++)
                        if (k < g) {
                            const bool b = (bm >> k) & 1u;
                            const unsigned long long m = wave_ballot(b);
                            const int slot = dg[k] + lanes_below(m);
                            if (b && slot < MMC_NET_MAX_DEG)
                                adj[((size_t)k * MMC_NET_MAX_DEG + slot) * n_mol + i] = (unsigned short)entry;
                            dg[k] += __popcll(m);
                        }
                };

                scan_candidates(sites, r, i, ci[0], ci[1], ci[2], bc, rmax2, cand, lane, [](int, bool, double) {}, bonds);
                if (lane == 0) {
#pragma unroll
                    for (int k = 0; k < MMC_NET_MAX_CRIT; k++)
                        if (k < g)
                            degc[(size_t)k * n_mol + i] = (unsigned char)min(dg[k], 255);
                }
            }

            // ---- clusters: one criterion after the other, all threads -------------------------------
            for (int k = 0; k < g; k++) {
                const int kk = k0 + k;
                const unsigned short *const a = adj + (size_t)k * n_mol * MMC_NET_MAX_DEG;
                const unsigned char *const dc = degc + (size_t)k * n_mol;
                const int64_t rk = (int64_t)r * K + kk;
                long long *const st = na.stats + rk * MMC_NET_STATS;
                int32_t *const lab_out = na.label ? na.label + rk * n_mol : nullptr;
                int32_t *const nbr_out = na.nbr ? na.nbr + rk * n_mol * MMC_NET_MAX_DEG : nullptr;

                __syncthreads(); // the lists are complete; the criterion before is done with the rest
                for (int q = tid; q < NET_RED; q += nt)
                    red[q] = 0u;
                for (int q = tid; q <= n_mol; q += nt)
                    shist[q] = 0u;
                __syncthreads();
                for (int i = tid; i < n_mol; i += nt) {
                    const unsigned d = dc[i];
                    if (d > MMC_NET_MAX_DEG)
                        red[NET_R_FLAG] = 1u;
                    else
                        atomicAdd(&red[d], 1u);
                }
                __syncthreads();
                if (red[NET_R_FLAG] != 0u) { // workgroup-uniform: the defined values, no histogram
                    if (tid < MMC_NET_STATS)
                        st[tid] = tid == 7 ? 1 : 0;
                    if (lab_out)
                        for (int i = tid; i < n_mol; i += nt)
                            lab_out[i] = -2;
                    if (nbr_out)
                        for (int q = tid; q < n_mol * MMC_NET_MAX_DEG; q += nt)
                            nbr_out[q] = -1;
                    continue;
                }
                if (na.deg_hist && tid <= MMC_NET_MAX_DEG && red[tid] != 0u)
                    atomicAdd(na.deg_hist + (ro * K + kk) * (MMC_NET_MAX_DEG + 1) + tid, (unsigned long long)red[tid]);

                // labels: every site its own index, offsets 0
                unsigned long long *cur = lab, *nxt = lab + n_mol;
                const int minb = na.min_bonds[kk];
                for (int i = tid; i < n_mol; i += nt)
                    cur[i] = (int)dc[i] >= minb ? ((unsigned long long)i << 48) | 0x800080008000ULL : ~0ULL;
                __syncthreads();
                for (int round = 0;; round++) {
                    if (tid == 0)
                        red[NET_R_CHANGED + (round + 1) % 3] = 0u;
                    bool changed = false;
                    for (int i = tid; i < n_mol; i += nt) {
                        const unsigned long long w = cur[i];
                        unsigned long long best = w;
                        const unsigned li = (unsigned)(w >> 48);
                        if (li != NET_NONE) {
                            const int n = dc[i]; // <= 16: nothing is flagged here
                            for (int e = 0; e < n; e++) {
                                const unsigned en = a[e * n_mol + i];
                                const unsigned long long wj = cur[en & 2047u];
                                if ((unsigned)(wj >> 48) < li) {
                                    const int c = (int)(en >> 11);
                                    const long long dm = ((long long)(c % 3 - 1)) + ((long long)(c / 3 % 3 - 1) << 16) +
                                                         ((long long)(c / 9 - 1) << 32);
                                    const unsigned long long cw = wj - (unsigned long long)dm; // offset_j - m_ij
                                    best = cw < best ? cw : best;
                                }
                            }
                        }
                        nxt[i] = best;
                        changed = changed || best != w;
                    }
                    if (changed)
                        red[NET_R_CHANGED + round % 3] = 1u;
                    __syncthreads();
                    unsigned long long *const sw = cur;
                    cur = nxt;
                    nxt = sw;
                    if (red[NET_R_CHANGED + round % 3] == 0u)
                        break;
                }

                // sizes and wrap masks by root, in the buffer the last round left free
                unsigned *const csz = reinterpret_cast<unsigned *>(nxt), *const cmk = csz + n_mol;
                for (int i = tid; i < n_mol; i += nt) {
                    csz[i] = 0u;
                    cmk[i] = 0u;
                }
                __syncthreads();
                for (int i = tid; i < n_mol; i += nt) {
                    const unsigned long long w = cur[i];
                    const unsigned li = (unsigned)(w >> 48);
                    if (li == NET_NONE)
                        continue;
                    atomicAdd(&csz[li], 1u);
                    const int n = dc[i];
                    unsigned mk = 0u;
                    for (int e = 0; e < n; e++) {
                        const unsigned en = a[e * n_mol + i];
                        const unsigned long long wj = cur[en & 2047u];
                        if ((unsigned)(wj >> 48) == NET_NONE)
                            continue;
                        const int c = (int)(en >> 11);
                        const int ex = (int)((w >> 0) & 0xFFFFu) + (c % 3 - 1) - (int)((wj >> 0) & 0xFFFFu);
                        const int ey = (int)((w >> 16) & 0xFFFFu) + (c / 3 % 3 - 1) - (int)((wj >> 16) & 0xFFFFu);
                        const int ez = (int)((w >> 32) & 0xFFFFu) + (c / 9 - 1) - (int)((wj >> 32) & 0xFFFFu);
                        mk |= (ex != 0 ? 1u : 0u) | (ey != 0 ? 2u : 0u) | (ez != 0 ? 4u : 0u);
                    }
                    if (mk != 0u)
                        atomicOr(&cmk[li], mk);
                }
                __syncthreads();
                for (int i = tid; i < n_mol; i += nt) {
                    if ((unsigned)(cur[i] >> 48) != (unsigned)i)
                        continue; // no root
                    const unsigned s = csz[i], mk = cmk[i];
                    atomicAdd(&shist[s], 1u);
                    atomicAdd(&red[NET_R_SITES], s);
                    atomicAdd(&red[NET_R_CLUSTERS], 1u);
                    atomicMax(&red[NET_R_LARGEST], s);
                    atomicAdd(&red[NET_R_S2], s * s);
                    if (mk != 0u) {
                        atomicOr(&red[NET_R_MASK], mk);
                        atomicMax(&red[NET_R_WRAPPING], s);
                    }
                }
                __syncthreads();
                if (tid == 0) {
                    unsigned twice = 0u;
                    for (int d = 1; d <= MMC_NET_MAX_DEG; d++)
                        twice += (unsigned)d * red[d];
                    st[0] = twice / 2u;
                    st[1] = red[NET_R_SITES];
                    st[2] = red[NET_R_CLUSTERS];
                    st[3] = red[NET_R_LARGEST];
                    st[4] = red[NET_R_S2];
                    st[5] = red[NET_R_MASK];
                    st[6] = red[NET_R_WRAPPING];
                    st[7] = 0;
                }
                if (na.size_hist)
                    for (int s = tid; s <= n_mol; s += nt) {
                        const unsigned v = shist[s];
                        if (v != 0u)
                            atomicAdd(na.size_hist + (ro * K + kk) * ((int64_t)n_mol + 1) + s, (unsigned long long)v);
                    }
                if (lab_out)
                    for (int i = tid; i < n_mol; i += nt) {
                        const unsigned li = (unsigned)(cur[i] >> 48);
                        lab_out[i] = li == NET_NONE ? -1 : (int)li;
                    }
                if (nbr_out)
                    for (int q = tid; q < n_mol * MMC_NET_MAX_DEG; q += nt)
                        nbr_out[q] = (q & (MMC_NET_MAX_DEG - 1)) < (int)dc[q >> 4]
                                         ? (int)(a[(q & (MMC_NET_MAX_DEG - 1)) * n_mol + (q >> 4)] & 2047u) : -1;
            }
        }
    }
}
