// mmc_units.inc -- host side of what the observable calls share.  Every one of them enqueues on the
// batch's one stream, drains it before it returns and keeps nothing on the device between calls, so
// one scratch buffer (mmc_batch::obs_buf) and one kind of call (ObsCall) serve them all:
//   the calls with one wavefront per (replica, molecule): mmc_batch_widom / _widom_at, _solute,
//   _solute_pair, _deletion and _forces (UnitsCall; the kernels' shared part is mmc_unit.hpp);
//   the pair passes over the i < j triangle: mmc_batch_rdf_sites, _orient_corr and _pair_energy
//   (tile_plan, tile_waves; the kernels' shared part is mmc_tiles.hpp), and mmc_batch_sdf on the
//   same tiles with a grid of its own per workgroup;
//   the neighbour scans: mmc_batch_local_order, _shell_order, _bond_order, _voronoi, _hbond_network,
//   _hbond_rings and _cavity / _cavity_at (min_box, stage_fits, nbr_launch; the kernels' shared part is
//   mmc_nbr.hpp);
//   and mmc_batch_dipoles, _structure_factor, _volume_perturb.
// At the end: what the insertion and solute calls share on the host (the temperature check, the Ewald
// self term, one solute's record, its refusals and the packer of its SOL_PAR rows).
// Included by mmc_hip.hip after mmc_batch.inc and before all of them.  DESIGN.md, "Unit kernels",
// "Tile passes" and "Neighbour scans".
#include "mmc_unit.hpp"
#include "mmc_tiles.hpp"

// preconditions of the read-only observables (those of mmc_batch_potential_ewald)
#define STRUCT_STATE(b)                                                                          \
    MMC_REQUIRE(!(b)->has_prev, MMC_ERR_STATE, "proposals outstanding: call mmc_batch_settle first"); \
    BATCH_NO_VOLUME_TRIAL(b)

// the 128-byte records where the batch keeps them in step with the coordinates (as the totals do)
static inline bool struct_use_rec(const mmc_batch *b)
{
    return b->sys.rec && b->sys.homogeneous && (b->sys.pb.on || b->fast_ok);
}

// Device scratch of the observable calls, kept on the batch and grown on demand (no allocation, and
// no device-wide synchronisation of a hipFree, per sample).
static int32_t obs_scratch(mmc_batch *b, size_t bytes, char **out)
{
    if (bytes > b->obs_bytes) {
        if (b->obs_buf)
            MMC_HIP(hipFree(b->obs_buf));
        b->obs_buf = nullptr;
        b->obs_bytes = 0;
        MMC_HIP(hipMalloc(&b->obs_buf, bytes));
        b->obs_bytes = bytes;
    }
    *out = static_cast<char *>(b->obs_buf);
    return MMC_OK;
}

// ... and the pinned staging of a unit call's per-replica block
static int32_t obs_staging(mmc_batch *b, size_t bytes, char **out)
{
    if (bytes > b->obs_host_bytes) {
        if (b->obs_host)
            MMC_HIP(hipHostFree(b->obs_host));
        b->obs_host = nullptr;
        b->obs_host_bytes = 0;
        MMC_HIP(hipHostMalloc(&b->obs_host, bytes, hipHostMallocDefault));
        b->obs_host_bytes = bytes;
    }
    *out = static_cast<char *>(b->obs_host);
    return MMC_OK;
}

// State (MMC_ERR_STATE), then scope (MMC_ERR_UNSUPPORTED) of a unit call; an entry point checks its
// arguments (MMC_ERR_ARG) first.
static int32_t units_state_scope(const mmc_batch *b, const char *what)
{
    MMC_REQUIRE(!b->has_prev, MMC_ERR_STATE, "proposals outstanding: call mmc_batch_settle first");
    BATCH_NO_VOLUME_TRIAL(b);
    MMC_REQUIRE(!b->needs_reload, MMC_ERR_STATE, "%s: a run failed half-way; set every replica again", what);
    BATCH_S_FRESH(b, what);
    BATCH_ONE_BOX(b, what);
    BATCH_NOT_WOLF(b, what);
    BATCH_NO_SOLUTE(b, what);
    MMC_REQUIRE(b->fast_ok, MMC_ERR_UNSUPPORTED,
                "%s: needs identical 3-atom molecules and a cutoff / kappa the erfc table covers", what);
    return MMC_OK;
}

// A selection of the batch's own molecules (deletion, forces).  The part that needs no batch, so
// that it is refused without a device ...
#define UNITS_SEL_ARG(n_sel, sel, what) MMC_REQUIRE(!(sel) || (n_sel) >= 1, MMC_ERR_ARG, "%s: n_sel must be >= 1", what)
// ... and the rest: h_sel = the caller's indices, or 0 .. N - 1 for sel == NULL
static int32_t units_selection(const mmc_batch *b, int32_t n_sel, const int32_t *sel, const char *what,
                               std::vector<int32_t> &h_sel)
{
    const int64_t R = b->sys.R, N = b->sys.n_mol;
    if (sel)
        for (int32_t k = 0; k < n_sel; k++)
            MMC_REQUIRE(sel[k] >= 0 && sel[k] < N, MMC_ERR_ARG, "%s: sel[%d] = %d outside 0..%lld", what, (int)k,
                        (int)sel[k], (long long)(N - 1));
    const int64_t n = sel ? (int64_t)n_sel : N;
    MMC_REQUIRE(R * n <= (int64_t)INT32_MAX, MMC_ERR_ARG, "%s: replicas x selected molecules exceeds 2^31 - 1", what);
    h_sel.resize((size_t)n);
    for (int64_t k = 0; k < n; k++)
        h_sel[k] = sel ? sel[k] : (int32_t)k;
    return MMC_OK;
}

// The minimum image of an atom pair from its molecules' (IMG) for one of the batch's own molecules,
// bounded by r_mol_max: exactly k_move_eval_wave's condition (mmc_batch.inc).
static bool units_image_by_molecule(const mmc_batch *b, const PairParams &pp)
{
    const DeviceSystem &s = b->sys;
    return b->rigid_only && b->image_by_molecule != 0 &&
           s.image_by_molecule(std::max(pp.lj_gate_sq, pp.qq_gate_sq)) &&
           s.pairs_inside_slack(pp.qq_gate_sq, pp.qq_slack_sq) && s.pairs_inside_slack(pp.lj_gate_sq, pp.lj_slack_sq);
}

// Persistent workgroups as k_move_eval_wave's launches (mmc_batch.inc), capped at option "wave_wgs"
// or at what is resident: occ waves on each of the 4 SIMDs of every compute unit.
static unsigned units_grid(const mmc_batch *b, int64_t n_units, int occ)
{
    const int64_t wgs = (n_units + WV_WAVES - 1) / WV_WAVES;
    const int64_t cap = b->wave_wgs > 0 ? b->wave_wgs : (int64_t)(4 * occ / WV_WAVES) * b->n_cus;
    return (unsigned)std::min(wgs, cap);
}

template <class Args>
using units_kernel_t = void (*)(BatchView, const double *, const double *, const int32_t *, FastConsts, PairParams, Args, int);

// One call's device scratch and its queue of work.  The scratch is laid out by take(): regions in the
// order they are asked for, each aligned to 256 bytes; what the kernels want zeroed is taken first
// and zero(n) clears the first n bytes.  Results come back through fetch(): a copy into host staging
// the call owns, and a memcpy into the caller's array that finish() makes only after MMC_OK.
// Between the first enqueue and finish() nothing returns: an error is kept in `e`, skips what
// follows, and finish() drains the stream whatever happened (the host buffers of copies already
// queued outlive them).
struct ObsCall {
    mmc_batch *b;
    hipStream_t st;
    size_t end = 0;
    char *base = nullptr;
    hipError_t e = hipSuccess;
    struct Out {
        void *dst; // the caller's array, or NULL: read through stage()'s pointer
        std::vector<char> h;
    };
    std::vector<Out> outs; // (growing it moves the vectors: their storage stays where the copies write)

    explicit ObsCall(mmc_batch *b_) : b(b_), st(b_->sys.stream) {}
    size_t take(size_t bytes)
    {
        const size_t o = end;
        end = o + ((bytes + 255) & ~(size_t)255);
        return o;
    }
    // after the last take()
    int32_t alloc() { return obs_scratch(b, end, &base); }
    template <class T> T *at(size_t off) const { return reinterpret_cast<T *>(base + off); }

    void copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
    {
        if (e == hipSuccess)
            e = hipMemcpyAsync(dst, src, bytes, kind, st);
    }
    void to_device(void *dst, const void *src, size_t bytes) { copy(dst, src, bytes, hipMemcpyHostToDevice); }
    void to_host(void *dst, const void *src, size_t bytes) { copy(dst, src, bytes, hipMemcpyDeviceToHost); }
    void zero(size_t n_bytes)
    {
        if (e == hipSuccess)
            e = hipMemsetAsync(base, 0, n_bytes, st);
    }
    // after a launch of the caller's own (which it skips unless e == hipSuccess)
    void launched()
    {
        if (e == hipSuccess)
            e = hipGetLastError();
    }
    // `bytes` at d_src into staging: the host copy, to be read after finish() returned MMC_OK
    const char *stage(const void *d_src, size_t bytes)
    {
        outs.push_back(Out{ nullptr, std::vector<char>(bytes) });
        to_host(outs.back().h.data(), d_src, bytes);
        return outs.back().h.data();
    }
    // ... and from there into the caller's array, when it gave one
    void fetch(void *user_dst, const void *d_src, size_t bytes)
    {
        if (!user_dst || !bytes)
            return;
        stage(d_src, bytes);
        outs.back().dst = user_dst;
    }
    int32_t finish(const char *what)
    {
        if (e == hipSuccess)
            e = hipStreamSynchronize(st);
        else
            (void)hipStreamSynchronize(st);
        MMC_REQUIRE(e == hipSuccess, MMC_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
        for (const Out &o : outs)
            if (o.dst)
                memcpy(o.dst, o.h.data(), o.h.size());
        return MMC_OK;
    }
};

// Waves per workgroup of a pass with per-wave counters in LDS: as many of TILE_WAVES as fit beside
// `fixed_bytes` in what a workgroup may ask for without opting in.
static int tile_waves(size_t fixed_bytes, size_t per_wave_bytes)
{
    int nw = TILE_WAVES;
    while (nw > 1 && fixed_bytes + (size_t)nw * per_wave_bytes > TILE_LDS_BYTES)
        nw >>= 1;
    return nw;
}

// Persistent workgroups of nw waves: four waves per SIMD of every compute unit (the passes are bound
// by vector issue and LDS atomics), or option "wave_wgs"; no more than give every wave a unit.
static unsigned obs_grid(const mmc_batch *b, int nw, int64_t n_units)
{
    const int64_t wgs = b->wave_wgs > 0 ? b->wave_wgs : (int64_t)(16 / nw) * b->n_cus;
    return (unsigned)std::max<int64_t>(1, std::min(wgs, (n_units + nw - 1) / nw));
}

// ---- the neighbour scans (mmc_nbr.hpp): local order, cavities, network, shell order, bond order,
// rings, Voronoi cells

// The smallest box of the batch's replicas: no radius of a scan may exceed half of it.
static double min_box(const DeviceSystem &s)
{
    return s.pb.on ? *std::min_element(s.pb.box.begin(), s.pb.box.end()) : s.bv.box;
}

// Are a replica's sites staged in LDS (24 bytes per molecule behind a workgroup's `fixed_bytes`)?
// Where they fit in `limit`, unless option "local_stage" is 0.
static bool stage_fits(const mmc_batch *b, size_t fixed_bytes, int64_t N, size_t limit)
{
    return b->local_stage && fixed_bytes + 24 * (size_t)N <= limit;
}

template <class Args>
using nbr_kernel_t = void (*)(BatchView, const double *, Args);

// One launch of a scan kernel on the call's stream: the records where the batch keeps them in step
// (struct_use_rec), dynamic LDS beyond what needs no opting in raised to lds_opt_in first.
template <class Args>
static void nbr_launch_one(ObsCall &oc, nbr_kernel_t<Args> k, bool use_rec, unsigned g, unsigned t, size_t lds, size_t lds_opt_in,
                           const Args &a)
{
    if (oc.e == hipSuccess && lds > TILE_LDS_BYTES)
        oc.e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_opt_in);
    if (oc.e == hipSuccess)
        k<<<g, t, lds, oc.st>>>(oc.b->sys.bv, use_rec ? oc.b->sys.rec : nullptr, a);
    oc.launched();
}
// K<REC, STAGE> of a kernel template K, given as pick(rec, stage) = K<decltype(rec)::value, decltype(stage)::value> ...
template <class Args, class Pick>
static void nbr_launch(ObsCall &oc, Pick pick, bool stage, unsigned g, unsigned t, size_t lds, size_t lds_opt_in, const Args &a)
{
    const bool use_rec = struct_use_rec(oc.b);
    const std::true_type T;
    const std::false_type F;
    const nbr_kernel_t<Args> k = use_rec ? (stage ? pick(T, T) : pick(T, F)) : (stage ? pick(F, T) : pick(F, F));
    nbr_launch_one(oc, k, use_rec, g, t, lds, lds_opt_in, a);
}
// ... and K<REC>, given as pick(rec)
template <class Args, class Pick>
static void nbr_launch(ObsCall &oc, Pick pick, unsigned g, unsigned t, size_t lds, size_t lds_opt_in, const Args &a)
{
    const bool use_rec = struct_use_rec(oc.b);
    const nbr_kernel_t<Args> k = use_rec ? pick(std::true_type()) : pick(std::false_type());
    nbr_launch_one(oc, k, use_rec, g, t, lds, lds_opt_in, a);
}

// gr.jl:87 on r^2, in the arithmetic of k_rdf: the bin of a squared distance
static inline double rdf_bin_of(double r2, double dr)
{
    return std::ceil(std::sqrt(r2) / dr);
}

// thr[k], k = 0 .. numbins: the largest double r^2 >= 0 with rdf_bin_of(r^2) <= k (the bin is
// monotone in r^2: sqrt, the division by dr > 0 and ceil are), found by bisection over the bit
// patterns of the non-negative doubles; thr[numbins + 1] = +inf.
static void rdf_thresholds(double dr, int numbins, std::vector<double> &thr)
{
    auto bits = [](double x) { uint64_t u; memcpy(&u, &x, 8); return u; };
    auto dbl = [](uint64_t u) { double x; memcpy(&x, &u, 8); return x; };
    thr.assign((size_t)numbins + 2, INFINITY);
    for (int k = 0; k <= numbins; k++) {
        const double e = dr * (k + 1);
        uint64_t lo = 0, hi = bits(e * e * 1.01); // bin(0) = 0 <= k; bin(hi) >= k + 2
        if (!(rdf_bin_of(dbl(hi), dr) > k)) {     // (dr so large that the bound overflowed: nothing is beyond)
            thr[k] = INFINITY;
            continue;
        }
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (rdf_bin_of(dbl(mid), dr) <= k)
                lo = mid;
            else
                hi = mid;
        }
        thr[k] = dbl(lo);
    }
}

// What a pass over the i < j triangle (mmc_tiles.hpp) takes from the batch, after its entry point
// refused what it can without one: the range against the boxes (MMC_ERR_ARG), the state, the size
// (MMC_ERR_UNSUPPORTED); then the bins -- gr.jl:5: dr = side / 2 / numbins, else the caller's range
// -- their thresholds and the tiles.  ta->thr and ta->per_replica are the caller's to set.
static int32_t tile_plan(const mmc_batch *b, int32_t numbins, double r_max, const char *what, TileArgs *ta,
                         std::vector<double> *thr)
{
    const DeviceSystem &s = b->sys;
    double min_box = s.bv.box;
    if (s.pb.on) {
        MMC_REQUIRE(r_max > 0.0, MMC_ERR_ARG, "%s: per-replica boxes have no common L/2: give r_max > 0", what);
        min_box = *std::min_element(s.pb.box.begin(), s.pb.box.end());
    }
    MMC_REQUIRE(!(r_max > 0.0) || r_max <= min_box / 2.0, MMC_ERR_ARG,
                "%s: r_max %g exceeds half of the smallest box %g", what, r_max, min_box);
    STRUCT_STATE(b);
    MMC_REQUIRE(s.n_mol >= 1 && s.n_mol <= (1 << 21), MMC_ERR_UNSUPPORTED,
                "%s: 1 .. 2^21 molecules (the tiles of a replica are counted in 32 bits)", what);
    // (a batch holds three-atom molecules only, mmc_batch_create: slots 0..2 exist in every molecule)
    const double dr = r_max > 0.0 ? r_max / numbins : (min_box / 2.0) / numbins;
    rdf_thresholds(dr, numbins, *thr);
    const int64_t K = (s.n_mol + 63) / 64;
    ta->box_r = s.pb.on ? s.pb.d_box : nullptr;
    ta->numbins = numbins;
    ta->inv_dr = (float)(1.0 / dr);
    ta->n_blocks = (int32_t)K;
    ta->tiles_per_rep = (int32_t)(K * (K + 1) / 2);
    ta->n_tiles = s.R * ta->tiles_per_rep;
    return MMC_OK;
}

// A unit call: an ObsCall whose scratch begins with rows [R n][row] of doubles, flags [R n], and the
// per-replica block: `per_rep` doubles and one count per replica ([R][per_rep] doubles, then [R] long
// long: sums the reduce kernel adds to or fills), then the S-buffer bits [R].  The block goes each
// way in one copy through pinned staging of the same layout.
struct UnitsCall : ObsCall {
    size_t R, nu, row_bytes, sums_bytes, blk_bytes;
    size_t o_rows, o_flags, o_blk;
    int per_rep;
    char *hblk = nullptr;

    UnitsCall(mmc_batch *b_, size_t n_units, int row, int per_rep_)
        : ObsCall(b_), R((size_t)b_->sys.R), nu(n_units), row_bytes(sizeof(double) * row * n_units),
          sums_bytes((sizeof(double) * per_rep_ + sizeof(long long)) * R), blk_bytes(sums_bytes + R), per_rep(per_rep_)
    {
        o_rows = take(row_bytes);
        o_flags = take(nu);
        o_blk = take(blk_bytes);
    }
    // after the last take(): the buffers, and the S-buffer bits into the staged block
    int32_t alloc()
    {
        MMC_TRY(ObsCall::alloc());
        MMC_TRY(obs_staging(b, blk_bytes, &hblk));
        memcpy(hblk + sums_bytes, b->s_cur.data(), R);
        return MMC_OK;
    }
    double *d_rows() const { return at<double>(o_rows); }
    uint8_t *d_flags() const { return at<uint8_t>(o_flags); }
    double *d_sums() const { return at<double>(o_blk); }
    long long *d_counts() const { return reinterpret_cast<long long *>(d_sums() + per_rep * R); }
    const uint8_t *d_scur() const { return at<uint8_t>(o_blk + sums_bytes); }
    double *h_sums() const { return reinterpret_cast<double *>(hblk); }
    long long *h_counts() const { return reinterpret_cast<long long *>(h_sums() + per_rep * R); }

    // the staged block, filled by the caller, to the device
    void upload_block() { to_device(base + o_blk, hblk, blk_bytes); }
    // the unit kernel: its IMG instantiation where img holds
    template <class Args>
    void launch(bool img, units_kernel_t<Args> k_img, units_kernel_t<Args> k_pair, int occ, const PairParams &pp, const Args &a)
    {
        if (e != hipSuccess)
            return;
        const DeviceSystem &s = b->sys;
        (img ? k_img : k_pair)<<<units_grid(b, (int64_t)nu, occ), WV_WAVES * 64, 0, st>>>(s.bv, s.rec, s.qq_tab, s.kpack, s.fc,
                                                                                         pp, a, (int)nu);
        e = hipGetLastError();
    }
    // the rows and flags the caller asked for into its vectors, the block's sums back into the
    // staging, and the stream drained; the caller's arrays are written only after MMC_OK
    int32_t finish(std::vector<double> *h_rows, std::vector<uint8_t> *h_flags, const char *what)
    {
        if (h_rows) {
            h_rows->resize(row_bytes / sizeof(double));
            to_host(h_rows->data(), d_rows(), row_bytes);
        }
        to_host(hblk, base + o_blk, sums_bytes);
        if (h_flags) {
            h_flags->resize(nu);
            to_host(h_flags->data(), d_flags(), nu);
        }
        return ObsCall::finish(what);
    }
};

// ---- what the insertion and solute calls share (mmc_widom.inc, mmc_solute.inc, mmc_solute_pair.inc,
// mmc_solute_chain.inc, mmc_deletion.inc); none of it needs a batch

static int32_t temperature_arg(double temperature, const char *what)
{
    MMC_REQUIRE(std::isfinite(temperature) && temperature > 0.0, MMC_ERR_ARG,
                "%s: temperature must be positive and finite", what);
    return MMC_OK;
}

// EwaldSelf of the charges q[n] alone, in orc_ewald_self's arithmetic (ewalds.jl:829-833): what a
// molecule's insertion adds to EwaldSelf(N) and its deletion takes away.
static double ewald_self_term(const double *q, int n, double kappa, double factor)
{
    double q2 = 0.0;
    for (int a = 0; a < n; a++)
        q2 += q[a] * q[a];
    return -kappa * q2 / std::sqrt(M_PI) * factor;
}

// One rigid solute as the calls take it: S sites, charge [S], eps and sig [S][3] against the three
// water slots, the body offsets [S][3] where the call draws the placements (else NULL), and the
// suffix of its arguments' names in messages ("", "_a", "_b").
struct SoluteIn {
    int32_t S;
    const double *offsets, *charge, *eps, *sig;
    const char *tag;
};

// The refusals of a solute, S in range: its NULL arrays (a caller checks the offsets or placements
// itself, in its own order) ...
static int32_t solute_null_args(const SoluteIn &u, const char *what)
{
    MMC_REQUIRE(u.charge, MMC_ERR_ARG, "%s: NULL charge%s", what, u.tag);
    MMC_REQUIRE(u.eps, MMC_ERR_ARG, "%s: NULL eps%s", what, u.tag);
    MMC_REQUIRE(u.sig, MMC_ERR_ARG, "%s: NULL sig%s", what, u.tag);
    return MMC_OK;
}
// ... and its values, the offsets where there are any.  *charged |= some charge is not zero,
// *q2 = sum q^2 in site order.
static int32_t solute_value_args(const SoluteIn &u, const char *what, bool *charged, double *q2)
{
    *q2 = 0.0;
    for (int a = 0; a < u.S; a++) {
        MMC_REQUIRE(std::isfinite(u.charge[a]), MMC_ERR_ARG, "%s: non-finite charge%s", what, u.tag);
        *charged = *charged || u.charge[a] != 0.0;
        *q2 += u.charge[a] * u.charge[a];
    }
    for (int q = 0; q < 3 * u.S; q++) {
        MMC_REQUIRE(std::isfinite(u.eps[q]) && u.eps[q] >= 0.0, MMC_ERR_ARG, "%s: eps%s must be finite and >= 0", what, u.tag);
        MMC_REQUIRE(std::isfinite(u.sig[q]) && u.sig[q] >= 0.0, MMC_ERR_ARG, "%s: sig%s must be finite and >= 0", what, u.tag);
        if (u.offsets)
            MMC_REQUIRE(std::isfinite(u.offsets[q]), MMC_ERR_ARG, "%s: non-finite offsets%s", what, u.tag);
    }
    return MMC_OK;
}

// The solute's rows of the parameter block the kernels read, par [S][SOL_PAR]: xyz [S][3] (the body
// offsets, or the sites of a fixed solute; NULL = zeros, the placements are the caller's), charge,
// eps (3), sig (3).
static void solute_pack(double *par, const SoluteIn &u, const double *xyz)
{
    for (int a = 0; a < u.S; a++) {
        double *p = par + SOL_PAR * a;
        for (int d = 0; d < 3; d++) {
            p[d] = xyz ? xyz[3 * a + d] : 0.0;
            p[4 + d] = u.eps[3 * a + d];
            p[7 + d] = u.sig[3 * a + d];
        }
        p[3] = u.charge[a];
    }
}
