// mmc_nbr.hpp -- what the per-molecule observables that start from an O-O scan of a replica share on
// the device: k_local_order_wave (mmc_local.hpp), k_hbond_network (mmc_network.hpp), k_shell_order_wave
// (mmc_shell.hpp), k_bond_qlm / k_bond_corr (mmc_bondorder.hpp) and k_voronoi_wave (mmc_voronoi.hpp);
// the host side (nbr_launch, stage_fits, min_box) is in mmc_units.inc and also serves k_cavity_lane
// (mmc_cavity.hpp) and k_hbond_rings (mmc_rings.hpp), which keep device copies of their own -- why is
// in DESIGN.md, "Neighbour scans".
//
// The sites.  One position per molecule, its O, read from the 128-byte records of homogeneous batches
// (REC) or from the SoA arrays, or, where the host found room (STAGE), from a copy of the replica in
// LDS: 24 bytes per molecule, SoA, so that consecutive lanes read consecutive doubles.  Sites is the accessor, stage_sites the copy with the
// two workgroup barriers around it.
//
// The run.  The UNIT is a molecule; a launch has `per` units in each of n_rep replicas, replica-major,
// and workgroup g of G takes the contiguous run [M g / G, M (g + 1) / G), M = n_rep per.  RunCursor splits it at the replica boundaries: the
// workgroup stages a replica once and its waves take the run's units of that replica in turn.
//
// The scans.  Lane l takes j = l, l + 64, ...: r^2 of d(centre, site j) through vector1D_abs (the same
// bits as the signed image squared; r^2 of d(O_j, O_i) is bit for bit r^2 of d(O_i, O_j), so one gate
// serves both directions of a pair).  scan_candidates appends the j inside a gate to a list that
// is worked off 64 at a time, one candidate per lane, and never overflows; scan_list appends
// (bits of r^2, j) to a list of NBR_CAP entries, or reports that there were more, and rank_sort then
// leaves neighbour k in lane k.  Both lists are in rising j.
//
// The bond.  HbPair holds u . v and |u|^2 |v|^2 of the four hydrogens of a pair of molecules; the
// test of one hydrogen against cos^2 is bonded().
//
// What a kernel does with a candidate or a neighbour, its counters, their layout and when they are
// flushed are its own.
#pragma once
#include "mmc_tiles.hpp"

#define NBR_WAVES TILE_WAVES         // waves per workgroup (fewer where the counters would not fit: tile_waves)
#define NBR_LDS_BYTES TILE_LDS_BYTES // dynamic LDS a workgroup may ask for without opting in
#define NBR_CAND 128                 // candidate slots per wave: at most 63 pending + 64 appended
#define NBR_CAP 64                   // neighbours in a sorted list: one lane each
#define NBR_LIST_BYTES (12 * NBR_CAP) // a wave's list: 64 keys, then 64 indices

// The O (slot 0) of molecule j of replica r: one 16-byte and one 8-byte load of the record, or the
// three arrays at first0[j].
template <bool REC>
__device__ __forceinline__ void load_oxygen3(const BatchView &bv, const double *__restrict__ rec, int r, int j,
                                             double &x, double &y, double &z)
{
    if constexpr (REC) {
        const double *p = rec + ((int64_t)r * bv.n_mol + j) * MMC_RSTRIDE;
        const double2 v0 = *reinterpret_cast<const double2 *>(p);
        x = v0.x; y = v0.y; z = p[2];
    } else {
        const int64_t a0 = (int64_t)r * bv.atom_stride + bv.first0[j];
        x = bv.ax[a0]; y = bv.ay[a0]; z = bv.az[a0];
    }
}

// The O of molecule j (j < n_mol) of replica r.  STAGE: from pos, the replica that stage_sites
// copied last.
template <bool REC, bool STAGE>
struct Sites {
    const BatchView &bv;
    const double *__restrict__ rec;
    double *pos; // [3][n_mol] in LDS

    __device__ __forceinline__ void get(int r, int j, double &x, double &y, double &z) const
    {
        const int n_mol = bv.n_mol;
        if constexpr (STAGE) {
            x = pos[j]; y = pos[n_mol + j]; z = pos[2 * n_mol + j];
        } else {
            load_oxygen3<REC>(bv, rec, r, j, x, y, z);
        }
    }
};

// Replica r's sites into s.pos by all threads of the workgroup.  The first barrier: every wave has
// left what the LDS held before.
template <bool REC, bool STAGE>
__device__ __forceinline__ void stage_sites(const Sites<REC, STAGE> &s, int r)
{
    const int n_mol = s.bv.n_mol;
    const Sites<REC, false> src{ s.bv, s.rec, nullptr };
    __syncthreads();
    for (int j = threadIdx.x; j < n_mol; j += (int)blockDim.x) {
        double x, y, z;
        src.get(r, j, x, y, z);
        s.pos[j] = x; s.pos[n_mol + j] = y; s.pos[2 * n_mol + j] = z;
    }
    __syncthreads();
}

// The run of this workgroup among n_rep replicas of `per` units, one replica at a time: units
// [lo, hi) of replica r (counted from the launch's first) after every next().
struct RunCursor {
    int64_t s0, s1;
    int per, r, lo, hi;

    __device__ __forceinline__ RunCursor(int n_rep, int per_)
        : s0((int64_t)n_rep * per_ * blockIdx.x / gridDim.x), s1((int64_t)n_rep * per_ * (blockIdx.x + 1) / gridDim.x),
          per(per_), r(0), lo(0), hi(0)
    {
    }
    __device__ __forceinline__ bool next()
    {
        if (s0 >= s1)
            return false;
        r = (int)(s0 / per);
        lo = (int)(s0 - (int64_t)r * per);
        hi = (int)min((int64_t)per, (int64_t)lo + (s1 - s0));
        s0 += hi - lo;
        return true;
    }
};

// The scan of molecule i's wave over the sites of replica r from the centre (cx, cy, cz).
// each(j, valid, r2) sees every lane's site of every pass (valid: j is a molecule other than i);
// the valid j with r2 < gate2 go to cand ([NBR_CAND], the wave's) in rising j, and body(n) is called
// with candidates [0, n), n <= 64, one per lane, in the list's first slots.
template <class S, class Each, class Body>
__device__ __forceinline__ void scan_candidates(const S &sites, int r, int i, double cx, double cy, double cz,
                                                const BoxConsts &bc, double gate2, int *cand, int lane, Each each, Body body)
{
    const int n_mol = sites.bv.n_mol;
    int n_cand = 0;
    for (int jb = 0; jb < n_mol; jb += 64) {
        const int j = jb + lane;
        const bool valid = j < n_mol && j != i;
        double x, y, z;
        sites.get(r, min(j, n_mol - 1), x, y, z);
        const double dx = vector1D_abs(cx, x, bc), dy = vector1D_abs(cy, y, bc), dz = vector1D_abs(cz, z, bc);
        const double r2 = (dx * dx + dy * dy) + dz * dz;
        each(j, valid, r2);
        const bool near = valid && r2 < gate2;
        const unsigned long long nm = wave_ballot(near);
        if (nm != 0ULL) { // wave-uniform
            if (near)
                cand[n_cand + lanes_below(nm)] = j; // n_cand <= 63 here: the slot is < NBR_CAND
            n_cand += __popcll(nm);
            wave_sync();
            if (n_cand >= 64) {
                body(64);
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
        body(n_cand);
    wave_sync(); // the list is rewritten by the wave's next molecule
}

// The same scan into a list of at most NBR_CAP: (bits of r^2, j) of the valid j with r2 < gate2 to
// keys / idx (the wave's), unsorted, in rising j; m of them.  A pass that would take the list beyond
// NBR_CAP ends the scan and nothing of it is written: the return value is false.
template <class S>
__device__ __forceinline__ bool scan_list(const S &sites, int r, int i, double cx, double cy, double cz, const BoxConsts &bc,
                                          double gate2, unsigned long long *keys, int *idx, int lane, int &m)
{
    const int n_mol = sites.bv.n_mol;
    bool over = false;
    m = 0;
    for (int jb = 0; jb < n_mol; jb += 64) {
        const int j = jb + lane;
        double x, y, z;
        sites.get(r, min(j, n_mol - 1), x, y, z);
        const double dx = vector1D_abs(cx, x, bc), dy = vector1D_abs(cy, y, bc), dz = vector1D_abs(cz, z, bc);
        const double r2 = (dx * dx + dy * dy) + dz * dz;
        const bool near = j < n_mol && j != i && r2 < gate2;
        const unsigned long long nm = wave_ballot(near);
        if (nm != 0ULL) { // wave-uniform
            const int add = __popcll(nm);
            if (m + add > NBR_CAP) { // more than the lanes can own: nothing written
                over = true;
                break;
            }
            if (near) {
                const int slot = m + lanes_below(nm); // < NBR_CAP
                keys[slot] = (unsigned long long)__double_as_longlong(r2);
                idx[slot] = j;
            }
            m += add;
        }
    }
    wave_sync();
    return !over;
}

// The list of scan_list sorted by (key, j): lane n < m takes entry n and counts the entries with a
// smaller key, and those before it with an equal one (the list is in rising j): its rank.  It writes
// its entry to that slot, and lane k then reads slot k: (key, jn) of neighbour k, (~0, -1) beyond m.
__device__ __forceinline__ void rank_sort(unsigned long long *keys, int *idx, int m, int lane, unsigned long long &key, int &jn)
{
    const bool mine = lane < m;
    key = mine ? keys[lane] : ~0ULL;
    jn = mine ? idx[lane] : -1;
    int rank = 0;
    for (int e = 0; e < m; e++) {
        const unsigned long long ke = keys[e]; // one address for the wave: a broadcast
        rank += (ke < key || (ke == key && e < lane)) ? 1 : 0;
    }
    wave_sync(); // every lane has read the unsorted list
    if (mine) {
        keys[rank] = key;
        idx[rank] = jn;
    }
    wave_sync();
    if (mine) {
        key = keys[lane];
        jn = idx[lane];
    }
    wave_sync(); // the list is rewritten by the wave's next molecule
}

// d(O, H_h) of a molecule's two hydrogens, c = its nine coordinates (O, H, H)
__device__ __forceinline__ void hb_arms(const double *c, const BoxConsts &bc, double (*u)[3])
{
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
        for (int d = 0; d < 3; d++)
            u[h][d] = vector1D(c[d], c[3 + 3 * h + d], bc);
}

// The hydrogen-bond geometry of molecules i and j (ci, cj: nine coordinates each; ui = hb_arms of i).
// v = d(O_i, O_j), w = d(O_j, O_i); hydrogen h = 0, 1 is i's (i donates to j), h = 2, 3 is j's:
// t[h] = u . v (or u . w), q[h] = |u|^2 |v|^2 (or |u|^2 |w|^2), u = d(O_donor, H).
struct HbPair {
    double vv, ww; // |v|^2, |w|^2: the same bits
    double t[4], q[4];
    unsigned code; // the boxes vector1D added to O_j - O_i: (m_x + 1) + 3 (m_y + 1) + 9 (m_z + 1)

    __device__ __forceinline__ HbPair(const double *ci, const double (*ui)[3], const double *cj, const BoxConsts &bc)
    {
        const double vx = vector1D(ci[0], cj[0], bc), vy = vector1D(ci[1], cj[1], bc), vz = vector1D(ci[2], cj[2], bc);
        vv = (vx * vx + vy * vy) + vz * vz;
        const double wx = vector1D(cj[0], ci[0], bc), wy = vector1D(cj[1], ci[1], bc), wz = vector1D(cj[2], ci[2], bc);
        ww = (wx * wx + wy * wy) + wz * wz;
        code = 0u;
#pragma unroll
        for (int d = 2; d >= 0; d--) {
            const double dd = cj[d] - ci[d];
            const unsigned m1 = fabs(dd) < bc.half ? 1u : (dd > 0.0 ? 0u : 2u);
            code = 3u * code + m1;
        }
#pragma unroll
        for (int h = 0; h < 2; h++) {
            t[h] = (ui[h][0] * vx + ui[h][1] * vy) + ui[h][2] * vz;
            q[h] = ((ui[h][0] * ui[h][0] + ui[h][1] * ui[h][1]) + ui[h][2] * ui[h][2]) * vv;
            const double ux = vector1D(cj[0], cj[3 + 3 * h], bc), uy = vector1D(cj[1], cj[4 + 3 * h], bc),
                         uz = vector1D(cj[2], cj[5 + 3 * h], bc);
            t[2 + h] = (ux * wx + uy * wy) + uz * wz;
            q[2 + h] = ((ux * ux + uy * uy) + uz * uz) * ww;
        }
    }
    // hydrogen h points at the acceptor within the cone: cos >= cos_hb, cos2 = cos_hb^2
    __device__ __forceinline__ bool bonded(int h, double cos2) const { return t[h] > 0.0 && t[h] * t[h] >= cos2 * q[h]; }
};
