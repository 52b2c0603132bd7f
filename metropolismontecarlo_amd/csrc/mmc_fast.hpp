// mmc_fast.hpp -- the production form of the per-move kernel (K1+K4) for the replica batch.
//
// Same results as k_move_eval (mmc_kernels.hpp), restructured around what rocprofv3 showed for it
// (profiles/round1_*): one workgroup per replica-move was latency- and occupancy-bound -- 189
// VGPRs (2 waves/SIMD), ~8 dependent memory round trips per workgroup (70 % of wave cycles in
// SQ_WAIT_ANY), move records read over PCIe, ocml erfc with 4 divergent ranges.
//
//   * topology is HOMOGENEOUS (every molecule has the same 3 atom types/charges, true for any
//     pure rigid-water system): neighbour types/charges/LJ parameters are launch constants,
//     no per-neighbour index loads;
//   * TWO memory round trips per workgroup.  Trip 1, issued together at entry: the move record
//     (which carries the chosen molecule's OLD and NEW coordinates, so nothing depends on it),
//     the first centres of mass of the COM scan, the erfc table, the k-vector constants.
//     Trip 2: the gather of the surviving neighbours' 96-byte records (atoms + COM) into an LDS
//     tile by 6 lanes x 16 B each ("LDS-staged neighbour tiles"), issued into registers and
//     overlapped with the reciprocal-space arithmetic; the pair loops then read LDS only;
//   * one lane per (neighbour, atom pair a-b): 9 lanes per neighbour, both states;
//   * erfc(kappa r)/r comes from a piecewise degree-9 polynomial in r^2, 16 pieces per octave
//     over r^2 in [0.25, 256), selected by the exponent/mantissa bits of r^2: no sqrt, no
//     division, no erfc in the loop.  The table (12.5 KB) is built once per kappa on the device
//     from ocml erfc/sqrt at Chebyshev nodes; its error against exact arithmetic is <= 3e-15
//     relative for kappa = 5.6/30 and <= 2e-14 up to kappa*r = 4 (tests/test_gpu_table.py) -- the
//     conditioning error of erfc(kappa*sqrt(r2)) in fp64, which the reference's own direct
//     evaluation carries too, is 5e-15 there;
//   * LJ terms (only atom pairs with eps > 0.001, energy.jl:270) run as a second compacted pass;
//   * move records are read from device memory (copied H2D on the stream), results are written
//     straight to pinned host memory.
//
// Branch decisions (gates, overlap, slack) still use the reference's exact comparisons on
// unfused arithmetic, so neighbour lists and overlap flags are bit-identical to the oracle's.
#pragma once
#include <type_traits>
#include "mmc_kernels.hpp"
#include "mmc_cand.hpp"

#define MMC_TILE 150      // neighbours staged per LDS tile (14 KB; doubles as reduction scratch)
#define MMC_REC 12        // doubles per molecule record: 9 atom coordinates + 3 COM
#define MMC_RSTRIDE 16    // doubles between records in HBM: every record is one 128-byte line
                          // (at a 96-byte stride half of them straddled two lines and a gather
                          // fetched 1.5 lines per record)
#define MMC_QQ_DEG 9
#define MMC_QQ_NCOEF (MMC_QQ_DEG + 1)
#define MMC_QQ_NINT 160   // 10 octaves [2^-2, 2^8) x 16 sub-intervals
#define MMC_QQ_NROW (MMC_QQ_NINT + 1) // ... after a row of zeros: where a masked-out evaluation lands
#define MMC_QQ_TABLE_DOUBLES (MMC_QQ_NROW * MMC_QQ_NCOEF)
__device__ __forceinline__ const double *pb_tab(const double *, int r, const PerBoxView &pb)
{
    return pb.tab + (int64_t)r * MMC_QQ_TABLE_DOUBLES;
}
#define MMC_QQ_UMIN 0.25
#define MMC_QQ_UMAX 256.0    // the host selects this kernel only if r_cut^2 + 100 <= UMAX,
#define MMC_QQ_XMAX 4.0      // kappa * sqrt(r_cut^2 + 100) <= XMAX (degree 9 is enough there)
#define MMC_QQ_KAPPA_MAX 0.5 // and kappa <= this (the series below UMIN needs kappa*r <= 0.25)
#define MMC_FLIST_CAP 768
#define MMC_PRE 3            // COM-scan iterations whose loads are issued at kernel entry: all of
                             // the scan at 750 molecules (3 x 256), so no second dependent trip
#define MMC_GATHER_REGS ((MMC_TILE * 6 + MMC_BLOCK - 1) / MMC_BLOCK)

// word offsets (8 B) inside a MoveRec
#define MV_COM_NEW 1
#define MV_AT_NEW 4
#define MV_COM_OLD 13
#define MV_AT_OLD 16
#define MV_Q_NEW 25
#define MV_WORDS 29
static_assert(sizeof(MoveRec) == MV_WORDS * 8, "MoveRec layout");
static_assert(MMC_TILE * MMC_REC >= 7 * MMC_BLOCK, "the tile doubles as reduction scratch");

// Launch constants of a homogeneous system (built on the host once, mmc_batch_create).
struct FastConsts {
    double qq9[9];             // q_a * q_b
    double ljp_eps[9], ljp_sig[9];
    int32_t ljp_ab[9];         // atom pairs (3a + b) with eps > 0.001 (energy.jl:270)
    int32_t n_ljp;
    double q[3];
    double eps9[9], sig9[9];   // the LJ table by atom pair 3a + b (k_move_eval_wave)
    int32_t qneg_mask;         // bit ab: q_a q_b < 0 (ewalds.jl:359, the overlap sentinel's pairs)
    int32_t lj_mask;           // bit ab: eps > 0.001 (energy.jl:270)
};

// Horner in t over one piece's 10 coefficients, read as five 16-byte pairs: ds_read_b128 moves
// twice the bytes per LDS cycle of the ds_read2_b64 an 8-byte aligned row gets (rows are 80 B, so
// every row is 16-byte aligned, and 16 consecutive rows start in 16 different bank groups).
__device__ __forceinline__ double qq_horner(const double *c, double t)
{
    static_assert(MMC_QQ_NCOEF == 10, "five coefficient pairs");
    const double2 *c2 = reinterpret_cast<const double2 *>(c);
    const double2 p4 = c2[4], p3 = c2[3], p2 = c2[2], p1 = c2[1], p0 = c2[0];
    double acc = p4.y;
    acc = fma(acc, t, p4.x);
    acc = fma(acc, t, p3.y);
    acc = fma(acc, t, p3.x);
    acc = fma(acc, t, p2.y);
    acc = fma(acc, t, p2.x);
    acc = fma(acc, t, p1.y);
    acc = fma(acc, t, p1.x);
    acc = fma(acc, t, p0.y);
    acc = fma(acc, t, p0.x);
    return acc;
}

// Row and offset d = u - (centre of the piece) from the bits of u: the piece is the exponent and
// the top 4 mantissa bits (piece 0 at u = 0.25), its centre those bits with the next one set --
// three instructions, and the subtraction is exact.  The coefficients of a row are those of the
// polynomial in t = d / (half width) in [-1, 1), scaled by the powers of the half width: a power of
// two, so Horner in d gives bit for bit what Horner in t gives on the unscaled coefficients
// (k_build_qq_table).  ROW 0 OF THE TABLE IS ALL ZEROS, piece i is row i + 1: a discarded
// evaluation is sent to row 0 (one select on the row offset, the inline constant 0).
__device__ __forceinline__ double qq_piece(double u, int &row)
{
    const unsigned hi = (unsigned)(__double_as_longlong(u) >> 32);
    row = (int)(hi >> 16) - (0x3FD0 - 1);
    const unsigned chi = (hi & 0xFFFF0000u) | 0x8000u;
    return u - __longlong_as_double((long long)((unsigned long long)chi << 32));
}

// f(u) = erfc(kappa*sqrt(u))/sqrt(u) on the piece that holds u: Horner in d.
__device__ __forceinline__ double qq_table_eval(const double *tab, double u)
{
    int row;
    const double t = qq_piece(u, row);
    return qq_horner(tab + row * MMC_QQ_NCOEF, t);
}

// The same with the row clamped into the table: for predicated callers that evaluate every lane
// and discard what lies outside [UMIN, UMAX) afterwards.
__device__ __forceinline__ double qq_table_eval_clamped(const double *tab, double u)
{
    int row;
    const double t = qq_piece(u, row);
    row = min(max(row, 1), MMC_QQ_NINT);
    return qq_horner(tab + row * MMC_QQ_NCOEF, t);
}

// ... with the discarding done by the table: a lane with keep == false evaluates the row of zeros,
// so the caller adds e * (q_a q_b) unconditionally -- e is +-0 there, and x + 0 * q == x bit for
// bit.  The caller guarantees u < UMAX where keep holds (the host selects these kernels only if
// the cutoffs lie inside the table); below UMIN the row saturates at 0 or 1 and the caller's
// series takes over.
__device__ __forceinline__ double qq_table_eval_masked(const double *tab, double u, bool keep)
{
    int row;
    const double t = qq_piece(u, row);
    row = keep ? min(max(row, 0), MMC_QQ_NINT) : 0;
    return qq_horner(tab + row * MMC_QQ_NCOEF, t);
}

// (keep as a lane mask in an SGPR pair, the way the wave kernels hold their gates: the select reads
// it directly.  Three instructions from the high word of u to the row's byte offset.)
__device__ __forceinline__ double qq_table_eval_lanes(const double *tab, double u, unsigned long long keep)
{
    const unsigned hi = (unsigned)(__double_as_longlong(u) >> 32);
    const unsigned chi = (hi & 0xFFFF0000u) | 0x8000u;
    const double t = u - __longlong_as_double((long long)((unsigned long long)chi << 32));
    unsigned row; // the high half of hi minus (0x3FD0 - 1), saturating at 0: one SDWA subtraction
    asm("v_sub_u32_sdwa %0, %1, %2 clamp dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:DWORD"
        : "=v"(row) : "v"(hi), "s"(0x3FD0u - 1u));
    unsigned off = __umul24(row, (unsigned)(MMC_QQ_NCOEF * sizeof(double)));
    asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(off) : "v"(off), "s"(keep));
    return qq_horner(reinterpret_cast<const double *>(reinterpret_cast<const char *>(tab) + off), t);
}

// u < UMIN happens only for like charges closer than 0.5 A (opposite charges that close are
// overlaps).  There x = kappa*r <= 0.25 and the Maclaurin series of erf needs 9 terms for 1e-16:
// erfc(x)/r = 1/r - (2 kappa/sqrt(pi)) * sum_n (-1)^n x^(2n) / (n! (2n+1)).
__device__ __forceinline__ double qq_pair(const double *tab, double u, double kappa)
{
    if (u >= MMC_QQ_UMIN)
        return qq_table_eval(tab, u);
    const double x2 = kappa * kappa * u;
    double p = 1.0 / (40320.0 * 17.0);
    p = fma(p, -x2, 1.0 / (5040.0 * 15.0));
    p = fma(p, -x2, 1.0 / (720.0 * 13.0));
    p = fma(p, -x2, 1.0 / (120.0 * 11.0));
    p = fma(p, -x2, 1.0 / (24.0 * 9.0));
    p = fma(p, -x2, 1.0 / (6.0 * 7.0));
    p = fma(p, -x2, 1.0 / (2.0 * 5.0));
    p = fma(p, -x2, 1.0 / 3.0);
    p = fma(p, -x2, 1.0);
    return rsqrt(u) - 1.1283791670955126 * kappa * p; // 2/sqrt(pi)
}

// The same series for callers that must not let its nine constants be hoisted out of their loop
// into registers (k_move_eval_wave): every coefficient is made opaque where it is used, so it is
// materialised inside the (cold) branch.
__device__ __forceinline__ double opaque_f64(double c)
{
    asm volatile("" : "+v"(c));
    return c;
}
__device__ __noinline__ double qq_pair_cold(double u, double kappa)
{
    const double x2 = kappa * kappa * u;
    double p = opaque_f64(1.0 / (40320.0 * 17.0));
    p = fma(p, -x2, opaque_f64(1.0 / (5040.0 * 15.0)));
    p = fma(p, -x2, opaque_f64(1.0 / (720.0 * 13.0)));
    p = fma(p, -x2, opaque_f64(1.0 / (120.0 * 11.0)));
    p = fma(p, -x2, opaque_f64(1.0 / (24.0 * 9.0)));
    p = fma(p, -x2, opaque_f64(1.0 / (6.0 * 7.0)));
    p = fma(p, -x2, opaque_f64(1.0 / (2.0 * 5.0)));
    p = fma(p, -x2, opaque_f64(1.0 / 3.0));
    p = fma(p, -x2, 1.0);
    return rsqrt(u) - opaque_f64(1.1283791670955126) * kappa * p; // 2/sqrt(pi)
}

// Build the table: one thread per piece.  Chebyshev interpolation at 11 nodes of the exact
// (ocml) function, converted to the monomial basis in t for Horner evaluation.
// Per-replica tables (a batch with per-replica boxes): grid (rows, R), replica r's table for
// kappa[r] at tab + r * MMC_QQ_TABLE_DOUBLES, only where mask[r] != 0 (mask NULL: every replica).
struct PerBoxTable {
    const double *kappa; // [R]
    const int32_t *mask; // [R] or NULL
};
__device__ __forceinline__ bool pb_table_replica(double &, double *&) { return true; }
__device__ __forceinline__ bool pb_table_replica(double &kappa, double *&tab, const PerBoxTable &pb)
{
    const int r = blockIdx.y;
    kappa = pb.kappa[r];
    tab += (int64_t)r * MMC_QQ_TABLE_DOUBLES;
    return !pb.mask || pb.mask[r];
}

// PerBox: empty = the one table of the batch, PerBoxTable = one per replica (mmc_batch_set_boxes).
// (A pack, not a flag: the one-box kernel keeps its argument block, and the offset of the hidden
// arguments behind it, exactly as they were.)
template <typename... PerBox>
__global__ void k_build_qq_table(double kappa, double *tab, PerBox... pb)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= MMC_QQ_NROW)
        return;
    if (!pb_table_replica(kappa, tab, pb...))
        return;
    if (idx == MMC_QQ_NINT) { // row 0: zeros (qq_table_eval_masked)
        for (int j = 0; j < MMC_QQ_NCOEF; j++)
            tab[j] = 0.0;
        return;
    }
    const int e = idx / 16 - 2, k = idx % 16;
    const double ua = ldexp(1.0 + k / 16.0, e), ub = ldexp(1.0 + (k + 1) / 16.0, e);
    const double uc = 0.5 * (ua + ub), uh = 0.5 * (ub - ua);
    const int N = MMC_QQ_NCOEF;
    double f[MMC_QQ_NCOEF], c[MMC_QQ_NCOEF];
    for (int n = 0; n < N; n++) {
        const double x = cos(3.141592653589793 * (n + 0.5) / N);
        const double u = uc + x * uh, r = sqrt(u);
        f[n] = erfc(kappa * r) / r;
    }
    for (int j = 0; j < N; j++) {
        double s = 0.0;
        for (int n = 0; n < N; n++)
            s += f[n] * cos(3.141592653589793 * j * (n + 0.5) / N);
        c[j] = s * (j == 0 ? 1.0 : 2.0) / N;
    }
    // Chebyshev -> monomial: T0 = 1, T1 = t, T_{j+1} = 2 t T_j - T_{j-1}
    double m[MMC_QQ_NCOEF], tp[MMC_QQ_NCOEF], tc[MMC_QQ_NCOEF], tn[MMC_QQ_NCOEF];
    for (int j = 0; j < N; j++) { m[j] = 0.0; tp[j] = 0.0; tc[j] = 0.0; }
    tp[0] = 1.0; // T0
    tc[1] = 1.0; // T1
    m[0] += c[0];
    for (int j = 0; j < N; j++)
        m[j] += c[1] * tc[j];
    for (int d = 2; d < N; d++) {
        for (int j = 0; j < N; j++)
            tn[j] = (j > 0 ? 2.0 * tc[j - 1] : 0.0) - tp[j];
        for (int j = 0; j < N; j++) {
            m[j] += c[d] * tn[j];
            tp[j] = tc[j];
            tc[j] = tn[j];
        }
    }
    // Horner runs in d = u - uc = t * uh, uh = 2^(e - 5): the scaling is exact
    for (int j = 0; j < N; j++)
        tab[(idx + 1) * N + j] = ldexp(m[j], -j * (e - 5));
}

// Evaluate the erfc(kappa r)/r approximation at arbitrary r^2 (accuracy tests, mmc_batch_qq_table).
__global__ void k_eval_qq_table(const double *tab, double kappa, const double *u, double *out,
                                int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        out[i] = qq_pair(tab, u[i], kappa);
}

// rec[r][j][0..8] = atoms of molecule j (x0 y0 z0 x1 ... z2), rec[r][j][9..11] = COM.
__global__ void k_build_rec(BatchView bv, double *rec, int r)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= bv.n_mol)
        return;
    double *o = rec + ((int64_t)r * bv.n_mol + j) * MMC_RSTRIDE;
    const int64_t a0 = r * bv.atom_stride + bv.first0[j], m0 = r * bv.mol_stride + j;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        o[3 * a] = bv.ax[a0 + a]; o[3 * a + 1] = bv.ay[a0 + a]; o[3 * a + 2] = bv.az[a0 + a];
    }
    o[9] = bv.comx[m0]; o[10] = bv.comy[m0]; o[11] = bv.comz[m0];
    comq_store(bv, r, j, 0, o[9]); comq_store(bv, r, j, 1, o[10]); comq_store(bv, r, j, 2, o[11]);
}

// (per_replica = n_mol * MMC_RSTRIDE doubles)
__global__ void k_broadcast_rec(double *rec, int64_t per_replica)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y + 1;
    if (i < per_replica)
        rec[r * per_replica + i] = rec[i];
}

__global__ void k_broadcast_f32(float *p, int64_t per_replica)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y + 1;
    if (i < per_replica)
        p[r * per_replica + i] = p[i];
}

// k-vector constants packed for one load per k: kx | (ky+5) << 4 | (kz+5) << 8 | column << 12, where
// `column` numbers the distinct (kx, ky) pairs in the order the k-vectors list them (50 of them for
// nk = 5, k^2 < 27; 63 stands for "past the 63rd").  The (kx, ky) of column c, packed the same way,
// is kpack[MMC_NK_STRIDE + c] (MMC_KCOLS entries, 0 past the last column): k_move_eval_wave builds
// the products e^{i kx x} e^{i ky y} of the moved atoms once per column, not once per k-vector.
// One block of MMC_NK_STRIDE threads.
#define MMC_KCOLS 64
__global__ void k_pack_kvec(const int32_t *kxyz, const int32_t *n_kvecs, int32_t *kpack)
{
    const int k = threadIdx.x, n = min(*n_kvecs, MMC_NK_STRIDE);
    if (k < MMC_KCOLS)
        kpack[MMC_NK_STRIDE + k] = 0;
    __syncthreads();
    if (k >= n) {
        if (k < MMC_NK_STRIDE)
            kpack[k] = 0;
        return;
    }
    auto key = [&](int j) { return kxyz[3 * j] * 16 + (kxyz[3 * j + 1] + 5); };
    int col = 0;
    for (int j = 1; j <= k; j++)
        col += key(j) != key(j - 1);
    const int xy = kxyz[3 * k] | ((kxyz[3 * k + 1] + 5) << 4);
    kpack[k] = xy | ((kxyz[3 * k + 2] + 5) << 8) | ((col < MMC_KCOLS - 1 ? col : MMC_KCOLS - 1) << 12);
    if (col < MMC_KCOLS && (k == 0 || key(k) != key(k - 1)))
        kpack[MMC_NK_STRIDE + col] = xy;
}

struct FastNoTables {};
template <bool PT> struct FastSharedT { // PT = false (WOLF): no phase tables
    alignas(16) double tile[MMC_TILE * MMC_REC]; // neighbour records, written as double2
    alignas(16) double mvw[MV_WORDS + 1];        // this replica's move record
    alignas(16) double pvw[MV_WORDS + 1];        // its previous move record (pending commit)
    alignas(16) double qtab[MMC_QQ_TABLE_DOUBLES];
    typename std::conditional<PT, cplx[2][3][3][MMC_NKTAB], FastNoTables>::type ptab;
    double red[7 * MMC_WAVES];
    double qq9[9], ljp_eps[9], ljp_sig[9];
    int32_t list[MMC_FLIST_CAP];
    int32_t tflag[MMC_TILE];
    int32_t ljp_ab[9];
    int32_t wcnt[MMC_WAVES];
    int32_t gflag;
};
typedef FastSharedT<true> FastShared;

// grid (n_parts, replicas of the group); same part semantics as k_move_eval.  PerBox: empty =
// the batch's one box; PerBoxView = replica r takes its box, kappa, cfac row and table from it
// (pb_* in mmc_kernels.hpp).
// WOLF = true (mmc_batch_set_coulomb_style; main.jl:75, :580-590): no reciprocal part -- no phase
// tables, no k-vector constants, neither S(k) buffer touched -- and every part of n_parts > 1 is a
// pair part.  Its own instantiation: the Ewald forms compile exactly as they did.
template <bool WOLF, typename... PerBox>
__global__ __launch_bounds__(MMC_BLOCK) void k_move_eval_fast(
    BatchView bv, double *rec, const double *qq_tab, const int32_t *kpack, FastConsts fc,
    const MoveRec *cur, const MoveRec *prev, PartOut *out, int n_parts, PairParams pp, int r_base,
    const uint8_t *flagv, unsigned stamp, PerBox... pb)
{
    __shared__ __align__(16) FastSharedT<!WOLF> sm;

    const int r = r_base + blockIdx.y, part = blockIdx.x, tid = threadIdx.x;
    const int n_mol = bv.n_mol;
    const double box = pb_box(bv, r, pb...);
    const double *comx = bv.comx + r * bv.mol_stride, *comy = bv.comy + r * bv.mol_stride,
                 *comz = bv.comz + r * bv.mol_stride;
    double *myrec = rec + (int64_t)r * n_mol * MMC_RSTRIDE;
    const bool do_pairs = WOLF ? true : (n_parts == 1) || (part < n_parts - 1);
    const bool do_recip = WOLF ? false : (n_parts == 1) || (part == n_parts - 1);
    const int np = WOLF ? n_parts : (n_parts == 1) ? 1 : n_parts - 1;
    const int plen = (n_mol + np - 1) / np;
    const int j_begin = do_pairs ? min(part * plen, n_mol) : 0;
    const int j_end = do_pairs ? min(j_begin + plen, n_mol) : 0; // >= j_begin
    const int w = wave_id();
    const BoxConsts bc = box_consts(box);

    // ================= trip 1: everything that depends on nothing =================
    if (tid < MV_Q_NEW)
        sm.mvw[tid] = reinterpret_cast<const double *>(cur + r)[tid];
    else if (prev && tid >= 32 && tid < 32 + MV_Q_NEW)
        sm.pvw[tid - 32] = reinterpret_cast<const double *>(prev + r)[tid - 32];
    else if (tid == 63)
        sm.gflag = flagv ? (int)flagv[r] : -1; // device-generated records: flags travel apart
    else if (tid >= 64 && tid < 73) {
        const int t = tid - 64;
        sm.qq9[t] = fc.qq9[t];
        sm.ljp_eps[t] = fc.ljp_eps[t];
        sm.ljp_sig[t] = fc.ljp_sig[t];
        sm.ljp_ab[t] = fc.ljp_ab[t];
    }
    if (do_pairs)
        for (int k = tid; k < MMC_QQ_TABLE_DOUBLES; k += MMC_BLOCK)
            sm.qtab[k] = pb_tab(qq_tab, r, pb...)[k];
    // first centres of mass of this wave's share of the COM scan
    const int len0 = min(MMC_FLIST_CAP, j_end - j_begin);
    const int seg0 = ((len0 + MMC_WAVES * 64 - 1) / (MMC_WAVES * 64)) * 64;
    // (the first MMC_PRE iterations of the scan: all of it for 750 molecules in one workgroup)
    double pcx[MMC_PRE], pcy[MMC_PRE], pcz[MMC_PRE];
    {
        const int w0 = j_begin + w * seg0, w1 = min(w0 + seg0, j_begin + len0);
#pragma unroll
        for (int it = 0; it < MMC_PRE; it++) {
            const int j = w0 + it * 64 + lane_id();
            pcx[it] = pcy[it] = pcz[it] = 0.0;
            if (do_pairs && j < w1) {
                pcx[it] = comx[j]; pcy[it] = comy[j]; pcz[it] = comz[j];
            }
        }
    }
    int kp0 = 0, kp1 = 0;
    double cf0 = 0.0, cf1 = 0.0;
    if (do_recip) {
        if (tid < bv.nkvecs) { kp0 = kpack[tid]; cf0 = pb_cfac(bv, r, pb...)[tid]; }
        if (tid + MMC_BLOCK < bv.nkvecs) { kp1 = kpack[tid + MMC_BLOCK]; cf1 = pb_cfac(bv, r, pb...)[tid + MMC_BLOCK]; }
    }
    __syncthreads();

    const int2 hdr = *reinterpret_cast<const int2 *>(&sm.mvw[0]);
    const int i0 = hdr.x - 1, flags = sm.gflag >= 0 ? sm.gflag : hdr.y;
    const bool commit = prev && (flags & 1);
    const int scur = (flags >> 1) & 1;
    const int pend = commit ? reinterpret_cast<const int *>(&sm.pvw[0])[0] - 1 : -1;
    // pending commit in record layout: word t of [atoms_new(9), com_new(3)]
    auto pd_word = [&](int t) { return sm.pvw[t < 9 ? MV_AT_NEW + t : MV_COM_NEW + (t - 9)]; };
    // chosen molecule: st 0 = old (from the host's mirror), st 1 = proposal
    auto ch_at = [&](int st, int a, int d) { return sm.mvw[(st ? MV_AT_NEW : MV_AT_OLD) + 3 * a + d]; };
    auto ch_com = [&](int st, int d) { return sm.mvw[(st ? MV_COM_NEW : MV_COM_OLD) + d]; };

    // commit of the previous accepted move (main.jl:598-621): written by one workgroup; every
    // reader in this launch substitutes the pending words for that molecule.
    if (part == 0 && commit && tid < 12) {
        const double v = pd_word(tid);
        myrec[(int64_t)pend * MMC_RSTRIDE + tid] = v;
        if (tid < 9) {
            const int a = tid / 3, d = tid % 3;
            (d == 0 ? bv.ax : d == 1 ? bv.ay : bv.az)[r * bv.atom_stride + 3 * pend + a] = v;
        } else {
            const int d = tid - 9;
            (d == 0 ? bv.comx : d == 1 ? bv.comy : bv.comz)[r * bv.mol_stride + pend] = v;
            pb_comq_store(bv, r, pend, d, v, pb...);
        }
    }
    if (part == 0 && commit && tid >= 12 && tid < 16)
        quat_commit(bv, r, pend, tid - 12, prev[r].q_new[tid - 12], quat_valid(prev[r].q_new));
    if constexpr (!WOLF)
    if (do_recip && tid >= 64 && tid < 82) { // phase tables of the 3 moved atoms, old and new
        const int t = tid - 64;
        const int st = t / 9, l = (t % 9) / 3, d = t % 3;
        phase_row(ch_at(st, l, d), box, sm.ptab[st][l][d]);
    }

    double a_lj0 = 0, a_lj1 = 0, a_v0 = 0, a_v1 = 0, a_q0 = 0, a_q1 = 0, a_rec = 0;
    int ovl0 = 0, ovl1 = 0;
    // S(k) of the current buffer for this thread's k-vectors: issued now, consumed after the pair
    // loops, so the round trip is hidden behind them
    double so0r = 0, so0i = 0, so1r = 0, so1i = 0;
    if (do_recip) {
        const double *So = s_buf(bv, r, scur);
        if (tid < bv.nkvecs) { so0r = So[2 * tid]; so0i = So[2 * tid + 1]; }
        if (tid + MMC_BLOCK < bv.nkvecs) {
            so1r = So[2 * (tid + MMC_BLOCK)]; so1i = So[2 * (tid + MMC_BLOCK) + 1];
        }
    }

    const int n_ljp = fc.n_ljp;
    // State of the current chunk of the molecule range (chunks of MMC_FLIST_CAP molecules; one
    // chunk at 750 molecules): list segment size and the four waves' survivor counts.
    int seg = 0, c0 = 0, c1 = 0, c2 = 0, c3 = 0, total = 0;

    // ---- phase A: COM gates of both states, survivors compacted into sm.list (ascending j) ----
    auto scan_chunk = [&](int jb, bool prefetched) {
        // A later chunk rewrites wcnt[] and the list: every wave must have read the previous
        // chunk's counts first (with an empty first chunk and no reciprocal part there is no
        // other barrier in between).
        if (jb != j_begin)
            __syncthreads();
        const int je = min(jb + MMC_FLIST_CAP, j_end);
        const int len = max(je - jb, 0);
        seg = ((len + MMC_WAVES * 64 - 1) / (MMC_WAVES * 64)) * 64;
        const int wj0 = jb + w * seg, wj1 = min(wj0 + seg, je);
        int count = 0;
        auto gate_and_append = [&](int j, double cx, double cy, double cz) {
            int f = 0;
            if (j < wj1 && j != i0) {
                if (j == pend) { cx = pd_word(9); cy = pd_word(10); cz = pd_word(11); }
#pragma unroll
                for (int st = 0; st < 2; st++) {
                    const double dx = vector1D(ch_com(st, 0), cx, bc);
                    const double dy = vector1D(ch_com(st, 1), cy, bc);
                    const double dz = vector1D(ch_com(st, 2), cz, bc);
                    const double r2 = dx * dx + dy * dy + dz * dz;
                    f |= (r2 < pp.lj_gate_sq) ? (1 << st) : 0;       // energy.jl:254
                    f |= (r2 < pp.qq_gate_sq) ? (4 << st) : 0;       // ewalds.jl:340
                }
            }
            const unsigned long long m = __ballot(f != 0);
            if (f)
                sm.list[w * seg + count + lanes_below(m)] = j | (f << 27);
            count += __popcll(m);
        };
        int base = wj0;
        if (prefetched) { // the iterations whose loads were issued at kernel entry
#pragma unroll
            for (int it = 0; it < MMC_PRE; it++) {
                if (base < wj1) {
                    gate_and_append(base + lane_id(), pcx[it], pcy[it], pcz[it]);
                    base += 64;
                }
            }
        }
        for (; base < wj1; base += 64) { // larger systems: plain loads
            const int j = base + lane_id();
            double cx = 0.0, cy = 0.0, cz = 0.0;
            if (j < wj1) { cx = comx[j]; cy = comy[j]; cz = comz[j]; }
            gate_and_append(j, cx, cy, cz);
        }
        if (lane_id() == 0)
            sm.wcnt[w] = count;
        __syncthreads();
        c0 = sm.wcnt[0]; c1 = sm.wcnt[1]; c2 = sm.wcnt[2]; c3 = sm.wcnt[3];
        total = c0 + c1 + c2 + c3;
    };

    // ---- trip 2: one 16-byte piece (of 6) of the record of the neighbour at list position t0 + n
    auto gather_piece = [&](int t0, int g, int &ent) {
        const int n = g / 6, piece = g - n * 6;
        const int pos = t0 + n;
        int slot;
        if (pos < c0) slot = pos;
        else if (pos < c0 + c1) slot = seg + (pos - c0);
        else if (pos < c0 + c1 + c2) slot = 2 * seg + (pos - c0 - c1);
        else slot = 3 * seg + (pos - c0 - c1 - c2);
        ent = sm.list[slot];
        const int j = ent & ((1 << 27) - 1);
        double2 v;
        if (j == pend) {
            v.x = pd_word(2 * piece);
            v.y = pd_word(2 * piece + 1);
        } else {
            v = *reinterpret_cast<const double2 *>(myrec + (int64_t)j * MMC_RSTRIDE + 2 * piece);
        }
        return v;
    };
    auto store_piece = [&](int g, double2 v, int ent) {
        const int n = g / 6, piece = g - n * 6;
        *reinterpret_cast<double2 *>(&sm.tile[n * MMC_REC + 2 * piece]) = v;
        if (piece == 0)
            sm.tflag[n] = ent >> 27;
    };

    // ---- the pair passes over the nt neighbours staged in sm.tile ----
    auto pair_passes = [&](int nt) {
        // Coulomb pass: one lane per (neighbour, a, b), both states.  Straight-line and
        // predicated: the two states' chains (minimum image -> r^2 -> table piece -> Horner) are
        // independent, so written without divergent regions they interleave and hide each
        // other's LDS / fp64 latency.  A term that the reference skips is added as +0.0, which
        // leaves the sum bit-identical.
        {
            int n = tid / 9, ab = tid - 9 * n; // g = 9 n + ab; g += 256 = 9*28 + 4
            for (int g = tid; g < nt * 9; g += MMC_BLOCK) {
                const int a = (ab * 11) >> 5, b = ab - 3 * a; // ab / 3, ab % 3 for ab < 9
                const int f = sm.tflag[n];
                const double bx = sm.tile[n * MMC_REC + 3 * b],
                             by = sm.tile[n * MMC_REC + 3 * b + 1],
                             bz = sm.tile[n * MMC_REC + 3 * b + 2];
                const double qq = sm.qq9[ab];
                double u[2];
#pragma unroll
                for (int st = 0; st < 2; st++) {
                    const double rx = vector1D(ch_at(st, a, 0), bx, bc);
                    const double ry = vector1D(ch_at(st, a, 1), by, bc);
                    const double rz = vector1D(ch_at(st, a, 2), bz, bc);
                    u[st] = rx * rx + ry * ry + rz * rz;
                }
                const bool g0 = (f & 4) != 0, g1 = (f & 8) != 0; // ewalds.jl:340 per state
                const bool ov0 = g0 && (u[0] < pp.ovr) && (qq < 0); // ewalds.jl:359
                const bool ov1 = g1 && (u[1] < pp.ovr) && (qq < 0);
                const bool in0 = g0 && !ov0 && (u[0] < pp.qq_slack_sq); // ewalds.jl:362
                const bool in1 = g1 && !ov1 && (u[1] < pp.qq_slack_sq);
                double e0 = qq_table_eval_clamped(sm.qtab, u[0]);
                double e1 = qq_table_eval_clamped(sm.qtab, u[1]);
                // like charges closer than 0.5 A: the series (practically never taken)
                if (__any((in0 && u[0] < MMC_QQ_UMIN) || (in1 && u[1] < MMC_QQ_UMIN))) {
                    if (u[0] < MMC_QQ_UMIN) e0 = qq_pair(sm.qtab, u[0], pb_kappa(pp.kappa, r, pb...));
                    if (u[1] < MMC_QQ_UMIN) e1 = qq_pair(sm.qtab, u[1], pb_kappa(pp.kappa, r, pb...));
                }
                a_q0 += in0 ? qq * e0 : 0.0;
                a_q1 += in1 ? qq * e1 : 0.0;
                ovl0 |= ov0 ? 1 : 0;
                ovl1 |= ov1 ? 1 : 0;
                n += 28;
                ab += 4;
                if (ab >= 9) { ab -= 9; n += 1; }
            }
        }
        // LJ pass: only atom pairs with eps > 0.001.  Items are dealt from the LAST thread down:
        // at ~117 neighbours the Coulomb pass leaves wave 0 a fifth, nearly empty iteration
        // (1044 = 4 x 256 + 20 items) while waves 2 and 3 are done after four -- they take the LJ
        // items (no barrier in between), so this pass hides behind wave 0's tail.
        for (int g = MMC_BLOCK - 1 - tid; g < nt * n_ljp; g += MMC_BLOCK) {
            int n = g, p = 0;
            if (n_ljp != 1) { // water has one LJ pair (O-O): skip the integer division
                n = g / n_ljp;
                p = g - n * n_ljp;
            }
            const int ab = sm.ljp_ab[p];
            const int a = ab / 3, b = ab - 3 * a;
            const int f = sm.tflag[n];
            const double e = sm.ljp_eps[p], sg = sm.ljp_sig[p];
            const double *t = &sm.tile[n * MMC_REC];
#pragma unroll
            for (int st = 0; st < 2; st++) {
                if (f & (1 << st)) {
                    const double rx = vector1D(ch_at(st, a, 0), t[3 * b], bc);
                    const double ry = vector1D(ch_at(st, a, 1), t[3 * b + 1], bc);
                    const double rz = vector1D(ch_at(st, a, 2), t[3 * b + 2], bc);
                    const double rab2 = rx * rx + ry * ry + rz * rz;
                    if (rab2 < pp.lj_slack_sq) {                 // energy.jl:270
                        const double cx = vector1D(ch_com(st, 0), t[9], bc);
                        const double cy = vector1D(ch_com(st, 1), t[10], bc);
                        const double cz = vector1D(ch_com(st, 2), t[11], bc);
                        const double s2 = sg * sg / rab2;
                        const double s6 = s2 * s2 * s2;
                        const double s12 = s6 * s6;
                        const double virab = e * (2.0 * s12 - s6);
                        const double f0 = rx * virab * s2, f1 = ry * virab * s2,
                                     f2 = rz * virab * s2;
                        const double pe = e * (s12 - s6);
                        const double pv = cx * f0 + cy * f1 + cz * f2;
                        if (st == 0) { a_lj0 += pe; a_v0 += pv; }
                        else { a_lj1 += pe; a_v1 += pv; }
                    }
                }
            }
        }
    };

    // ===== chunk 0: scan, REQUEST the first neighbour tile into registers, do the reciprocal part
    // while that round trip is in flight, then stage the tile and run the pair passes =====
    scan_chunk(j_begin, true);
    {
        double2 greg[MMC_GATHER_REGS];
        int gent[MMC_GATHER_REGS];
        const int nt0 = min(MMC_TILE, total);
#pragma unroll
        for (int q = 0; q < MMC_GATHER_REGS; q++) {
            const int g = tid + q * MMC_BLOCK;
            gent[q] = 0;
            greg[q] = make_double2(0.0, 0.0);
            if (g < nt0 * 6)
                greg[q] = gather_piece(0, g, gent[q]);
        }
        // ---- reciprocal part for this thread's k-vectors (ewalds.jl:803-821) ----
        if constexpr (!WOLF)
        if (do_recip) {
            __syncthreads(); // ptab
            double *Sn = s_buf(bv, r, scur ^ 1);
#pragma unroll 1
            for (int h = 0; h < 2; h++) {
                const int k = tid + h * MMC_BLOCK;
                if (k < bv.nkvecs) {
                    const int kp = h ? kp1 : kp0;
                    const double cf = h ? cf1 : cf0;
                    const double orr = h ? so1r : so0r, oi = h ? so1i : so0i;
                    const int kx = kp & 15, ky = (kp >> 4) & 15, kz = (kp >> 8) & 15;
                    double nr = orr, ni = oi;
#pragma unroll 1
                    for (int l = 0; l < 3; l++) {
                        const cplx tn = c_mul(c_mul(sm.ptab[1][l][0][5 + kx], sm.ptab[1][l][1][ky]),
                                              sm.ptab[1][l][2][kz]);
                        const cplx to = c_mul(c_mul(sm.ptab[0][l][0][5 + kx], sm.ptab[0][l][1][ky]),
                                              sm.ptab[0][l][2][kz]);
                        nr += fc.q[l] * (tn.re - to.re);
                        ni += fc.q[l] * (tn.im - to.im);
                    }
                    Sn[2 * k] = nr; Sn[2 * k + 1] = ni;
                    a_rec += cf * ((nr * nr - (-ni) * ni) - (orr * orr - (-oi) * oi));
                }
            }
        }
        if (nt0 > 0) {
#pragma unroll
            for (int q = 0; q < MMC_GATHER_REGS; q++) {
                const int g = tid + q * MMC_BLOCK;
                if (g < nt0 * 6)
                    store_piece(g, greg[q], gent[q]);
            }
            __syncthreads();
            pair_passes(nt0);
            __syncthreads(); // the tile and the list are reused
        }
    }
    // ===== everything beyond the first tile: only systems with more than MMC_TILE neighbours
    // inside the gate or more than MMC_FLIST_CAP molecules per part get here =====
    {
        int jb = j_begin, t0 = MMC_TILE;
        for (;;) {
            if (t0 >= total) {
                jb += MMC_FLIST_CAP;
                if (jb >= j_end)
                    break;
                scan_chunk(jb, false);
                t0 = 0;
                continue;
            }
            const int nt = min(MMC_TILE, total - t0);
            for (int g = tid; g < nt * 6; g += MMC_BLOCK) {
                int ent;
                const double2 v = gather_piece(t0, g, ent);
                store_piece(g, v, ent);
            }
            __syncthreads();
            pair_passes(nt);
            __syncthreads();
            t0 += MMC_TILE;
        }
    }

    // one transpose-reduction for the seven sums and the two overlap flags; the tile is free now
    __syncthreads();
    double v[7] = { a_lj0, a_lj1, a_v0, a_v1, a_q0, a_q1, a_rec };
    block_sum_wide<7>(v, sm.tile, sm.red, ovl0 | (ovl1 << 1), sm.wcnt);
    if (tid == 0) { // sm.red[0..6] are already in PartOut order
        const int of = sm.wcnt[0] | sm.wcnt[1] | sm.wcnt[2] | sm.wcnt[3];
        sm.red[7] = pack_ovl(of & 1, (of >> 1) & 1, stamp, part_checksum(sm.red, stamp));
    }
    __syncthreads();
    store_part(out + (int64_t)r * n_parts + part, sm.red, tid);
}

// settle for the record layout: as k_settle, plus rec.  `cv`: the batch's candidate lists (mmc_cand.hpp;
// cv.idx NULL: none) -- the commit raises the replica's displacement bound, so that a call does not end
// by invalidating its lists.
__global__ void k_settle_rec(BatchView bv, double *rec, const MoveRec *prev,
                             const int32_t *accept, int r_base, int nr, CandView cv)
{
    const int q = blockIdx.x * 16 + (threadIdx.x >> 4), t = threadIdx.x & 15;
    const int r = r_base + q;
    if (q >= nr || !accept[r] || t >= 13)
        return;
    const int m = prev[r].mol - 1;
    if (t == 12) { // (one lane per replica, the only writer of D_r while this kernel runs)
        if (cv.idx && bv.comq) {
            const double inv_box = 1.0 / bv.box;
            const uint32_t xy = (uint32_t)com_quant(prev[r].com_new[0], inv_box)
                                | (uint32_t)com_quant(prev[r].com_new[1], inv_box) << 16;
            cand_note_commit(cv, cand_q0_xy(cv, bv.cq_stride, r, m), cand_q0_z(cv, bv.cq_stride, r, m), r, xy,
                             (uint32_t)com_quant(prev[r].com_new[2], inv_box), cv.D[r], true);
        }
        return;
    }
    const double v = (t < 9) ? prev[r].atoms_new[t] : prev[r].com_new[t - 9];
    rec[((int64_t)r * bv.n_mol + m) * MMC_RSTRIDE + t] = v;
    if (t >= 9)
        comq_store(bv, r, m, t - 9, v);
}
