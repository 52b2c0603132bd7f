// mmc_units.inc -- host side of what the calls with one wavefront per (replica, molecule) share:
// mmc_batch_widom / _widom_at (mmc_widom.inc), mmc_batch_deletion (mmc_deletion.inc) and
// mmc_batch_forces (mmc_forces.inc); the kernels' shared part is mmc_unit.hpp.  Included by
// mmc_hip.hip after mmc_batch.inc and before the three.  DESIGN.md, "Unit kernels".
//
// obs_scratch is also the device scratch of mmc_struct.inc, mmc_local.inc and mmc_vperturb.inc: every
// observable call enqueues on the batch's one stream, drains it before it returns with success and
// keeps nothing in the buffer between calls, so one buffer (mmc_batch::obs_buf) serves them all.
#include "mmc_unit.hpp"

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
// order they are asked for, each aligned to 256 bytes.  Every unit call has rows [R n][row] of
// doubles first, flags [R n], and the per-replica block: `per_rep` doubles and one count per replica
// ([R][per_rep] doubles, then [R] long long: sums the reduce kernel adds to or fills), then the
// S-buffer bits [R].  The block goes each way in one copy through pinned staging of the same layout.
// Between the first enqueue and finish() nothing returns: an error is kept in `e`, skips what
// follows, and finish() drains the stream whatever happened (the host buffers of copies already
// queued outlive them).
struct UnitsCall {
    mmc_batch *b;
    hipStream_t st;
    size_t R, nu, row_bytes, sums_bytes, blk_bytes;
    size_t end = 0, o_rows, o_flags, o_blk;
    int per_rep;
    char *base = nullptr, *hblk = nullptr;
    hipError_t e = hipSuccess;

    UnitsCall(mmc_batch *b_, size_t n_units, int row, int per_rep_)
        : b(b_), st(b_->sys.stream), R((size_t)b_->sys.R), nu(n_units), row_bytes(sizeof(double) * row * n_units),
          sums_bytes((sizeof(double) * per_rep_ + sizeof(long long)) * R), blk_bytes(sums_bytes + R), per_rep(per_rep_)
    {
        o_rows = take(row_bytes);
        o_flags = take(nu);
        o_blk = take(blk_bytes);
    }
    size_t take(size_t bytes)
    {
        const size_t o = end;
        end = o + ((bytes + 255) & ~(size_t)255);
        return o;
    }
    // after the last take(): the buffers, and the S-buffer bits into the staged block
    int32_t alloc()
    {
        MMC_TRY(obs_scratch(b, end, &base));
        MMC_TRY(obs_staging(b, blk_bytes, &hblk));
        memcpy(hblk + sums_bytes, b->s_cur.data(), R);
        return MMC_OK;
    }
    template <class T> T *at(size_t off) const { return reinterpret_cast<T *>(base + off); }
    double *d_rows() const { return at<double>(o_rows); }
    uint8_t *d_flags() const { return at<uint8_t>(o_flags); }
    double *d_sums() const { return at<double>(o_blk); }
    long long *d_counts() const { return reinterpret_cast<long long *>(d_sums() + per_rep * R); }
    const uint8_t *d_scur() const { return at<uint8_t>(o_blk + sums_bytes); }
    double *h_sums() const { return reinterpret_cast<double *>(hblk); }
    long long *h_counts() const { return reinterpret_cast<long long *>(h_sums() + per_rep * R); }

    void copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
    {
        if (e == hipSuccess)
            e = hipMemcpyAsync(dst, src, bytes, kind, st);
    }
    void to_device(void *dst, const void *src, size_t bytes) { copy(dst, src, bytes, hipMemcpyHostToDevice); }
    void to_host(void *dst, const void *src, size_t bytes) { copy(dst, src, bytes, hipMemcpyDeviceToHost); }
    // the staged block, filled by the caller, to the device
    void upload_block() { to_device(base + o_blk, hblk, blk_bytes); }
    // after a launch of the caller's own
    void launched()
    {
        if (e == hipSuccess)
            e = hipGetLastError();
    }
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
        if (e == hipSuccess)
            e = hipStreamSynchronize(st);
        else
            (void)hipStreamSynchronize(st);
        MMC_REQUIRE(e == hipSuccess, MMC_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
        return MMC_OK;
    }
};
