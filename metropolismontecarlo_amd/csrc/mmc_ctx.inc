// mmc_ctx.inc -- the context API: one system on one GPU behind the reference's per-call surface.
// Included by mmc_hip.hip.
//
// The reference's Loop() (Ewald/main.jl:487-644) mutates host arrays between calls and calls the
// hot path five times per trial move.  A context keeps
//   * a host MIRROR of the coordinates as the caller last showed them (mmc_set_molecule, or the
//     mmc_call_* entry points, which look at the caller's own arrays) and a list of the molecules
//     whose device copy is stale -- they travel with the next evaluation instead of a launch each;
//   * the last per-molecule evaluation (LJ and real-space Coulomb are always computed together),
//     keyed by molecule, cutoffs and a version number of the mirror: the second of LJ_poly_dU(i) /
//     EwaldShort(i) on an unchanged system is answered from it without touching the device;
//   * a speculative RecipMove, computed in the same command as the evaluation of a molecule whose
//     old coordinates the device still holds, into a free structure-factor buffer;
//   * for homogeneous 3-site systems the persistent server of mmc_ctxsrv.hpp, which answers a
//     command in a few microseconds instead of a launch + stream synchronisation (~18 us).
// Nothing here computes an energy on the host.
#include "mmc_ctxsrv.hpp"
#include <atomic>
#include <chrono>

#define CTX_NSBUF 4 // structure-factor buffers of a context: old, new, a speculative one, a spare

struct CtxDirty {
    int32_t mol;        // 0-based
    double dev_rec[12]; // what the device holds for it: atoms (9) + com (3); 3-atom molecules only
    bool has_dev_rec;
};

struct CtxEval { // one per-molecule evaluation, raw sums (energy.jl:289 / ewalds.jl:375 not applied)
    double lj_pot[2], lj_vir[2], qq_pot[2]; // [old, new]; one-state evaluations fill [1]
    int32_t ovl[2];
    double recip;           // sum_k cfac (|S_dst|^2 - |S_base|^2), no factor
    unsigned long long s_sum;
};

struct mmc_ctx {
    DeviceSystem sys;
    // trial-move state (mmc_trial_move / mmc_accept_move / mmc_reject_move)
    MoveRec *h_move = nullptr, *d_move = nullptr; // pinned, mapped
    PartOut *h_parts = nullptr, *d_parts = nullptr;
    bool trial_outstanding = false;
    int32_t trial_overlap = 0;
    int64_t trial_mol = 0;
    int n_parts = 1;

    // ---- host mirror of the coordinates and what the device lacks ----
    std::vector<double> m_com, m_at; // [n_mol][3], [n_atoms][3]: the caller's arrays at the last sync
    std::vector<CtxDirty> dirty;
    uint64_t version = 1;            // of the mirror
    int64_t last_call_mol = 0;       // molecule (1-based) of the last mmc_call_* (0: none)

    // ---- last per-molecule evaluation ----
    struct {
        bool valid = false;
        int64_t mol = 0;
        uint64_t version = 0;
        double lj_rcut = 0, qq_rcut = 0, ovr = 0;
        bool has_lj = false, has_qq = false;
        double lj_pot = 0, lj_vir = 0, qq_pot = 0;
        int32_t ovl = 0;
    } ec;
    double last_lj_rcut = 0, last_qq_rcut = 0; // the cutoff to assume for the term not asked for

    // ---- structure-factor buffers: which holds sumQExpOld / sumQExpNew ----
    int s_old = 0, s_new = 0;               // buffer indices; equal when the two arrays are equal
    bool m_valid[CTX_NSBUF] = { false, false, false, false }; // host mirror of buffer b is current
    struct { // speculative RecipMove of the last evaluation
        bool valid = false;
        double r_old[9], r_new[9], q[3];
        int base = 0, dst = 0;
        double dE = 0; // no factor
    } rc;
    struct { // look-ahead: the evaluation of the molecule expected next, riding on the last command
        bool posted = false;
        int64_t mol = 0;          // 1-based
        uint64_t version = 0;     // of the mirror when it was posted
        unsigned stamp = 0;
        int64_t launch = 0;       // srv.n_launches at the time (a replaced server never ran it)
        double lj_rcut = 0, qq_rcut = 0, ovr = 0;
    } la;
    int64_t n_la_hits = 0, n_la_posted = 0;
    struct { // the molecule of the last speculative RecipMove and where it went (hint only)
        bool valid = false;
        int32_t mol = 0;
        double new_rec[12];
    } prev_trial;

    // ---- persistent server (mmc_ctxsrv.hpp) ----
    struct {
        bool alive = false;
        int G = 1, wpg = SRV_WAVES, P = SRV_WAVES; // workgroups, waves each, records the host waits for
        bool lat = false;                          // k_ctx_server_lat (one record per workgroup)
        bool look_ahead = false;                   // ... launched with its look-ahead workgroups
        double lj_rcut = 0, qq_rcut = 0, ovr = 0, kappa = 0, box = 0;
        hipStream_t stream = nullptr;
        unsigned long long *h_cmd = nullptr, *d_cmd = nullptr;
        unsigned long long *bar_cmd = nullptr; // the block the server polls when the device has a large
                                               // BAR (mmc_bar_alloc): h_cmd is then the host's staging copy
        PartOut *h_out = nullptr, *d_out = nullptr;
        int32_t *h_state = nullptr, *d_state = nullptr;
        double *h_smir = nullptr, *d_smir = nullptr; // [CTX_NSBUF][2 * MMC_NK_STRIDE]
        unsigned long long seq = 0; // last sequence number posted
        unsigned stamp = 0;
        std::chrono::steady_clock::time_point last_post;
        int64_t n_cmds = 0, n_launches = 0, n_retries = 0;
    } srv;
    int64_t n_cache_hits = 0, n_spec_hits = 0, n_spec_miss = 0, n_launch_evals = 0;
    int server_mode = -1; // -1: use the server when it applies, 0: never (launch per evaluation)

    // ---- volume move (mmc_volume_trial / accept / reject) ----
    std::vector<double> mirror_scale; // factors the device has applied to its coordinates and the
                                      // host mirror has not yet (k_rescale's arithmetic, lazily)
    struct {
        bool outstanding = false;
        size_t n_scale = 0; // mirror_scale.size() before the trial
        int s_old = 0, s_new = 0;
        bool m_valid[CTX_NSBUF] = { false, false, false, false };
    } vol;
};

#define CTX_CHECK(ctx)                                                                           \
    MMC_REQUIRE((ctx) != nullptr, MMC_ERR_ARG, "ctx is NULL");                                   \
    MMC_HIP(hipSetDevice((ctx)->sys.device))

// Between mmc_volume_trial and its accept / reject the context holds the TRIAL volume and a
// snapshot to go back to: nothing that reads or writes coordinates, the host mirror or S(k) may run
// in between (it would apply the trial's scale factor to the mirror, which a reject cannot undo).
#define CTX_NO_VOLUME_TRIAL(ctx)                                                                 \
    MMC_REQUIRE(!(ctx)->vol.outstanding, MMC_ERR_STATE,                                          \
                "volume move not settled: call mmc_volume_accept or mmc_volume_reject first")

#define CTX_MOL(ctx, i)                                                                          \
    MMC_REQUIRE((ctx)->sys.uploaded, MMC_ERR_STATE, "no system uploaded");                       \
    MMC_REQUIRE((i) >= 1 && (i) <= (ctx)->sys.n_mol, MMC_ERR_ARG,                                \
                "molecule index %lld outside 1..%lld", (long long)(i),                           \
                (long long)(ctx)->sys.n_mol)

static int32_t ctx_pinned(void **h, void **d, size_t bytes)
{
    MMC_HIP(hipHostMalloc(h, bytes, hipHostMallocMapped | hipHostMallocCoherent));
    MMC_HIP(hipHostGetDevicePointer(d, *h, 0));
    memset(*h, 0, bytes);
    return MMC_OK;
}

extern "C" int32_t mmc_ctx_create(int32_t device, void *hip_stream, mmc_ctx **out)
{
    MMC_REQUIRE(out, MMC_ERR_ARG, "out is NULL");
    *out = nullptr;
    mmc_ctx *c = new mmc_ctx();
    int32_t st = c->sys.init(device, hip_stream, 1);
    if (st == MMC_OK)
        st = ctx_pinned((void **)&c->h_move, (void **)&c->d_move, sizeof(MoveRec));
    if (st == MMC_OK)
        st = ctx_pinned((void **)&c->h_parts, (void **)&c->d_parts, sizeof(PartOut) * 64);
    if (st == MMC_OK)
        st = ctx_pinned((void **)&c->srv.h_cmd, (void **)&c->srv.d_cmd, sizeof(unsigned long long) * 64);
    if (st == MMC_OK)
        c->srv.bar_cmd = (unsigned long long *)mmc_bar_alloc(sizeof(unsigned long long) * 64); // (may be NULL)
    if (st == MMC_OK)
        st = ctx_pinned((void **)&c->srv.h_out, (void **)&c->srv.d_out, sizeof(PartOut) * (CS_OUT_RECORDS > MMC_MAX_PARTS ? CS_OUT_RECORDS : MMC_MAX_PARTS));
    if (st == MMC_OK)
        st = ctx_pinned((void **)&c->srv.h_state, (void **)&c->srv.d_state, 512);
    if (st == MMC_OK)
        st = ctx_pinned((void **)&c->srv.h_smir, (void **)&c->srv.d_smir,
                        sizeof(double) * 2 * MMC_NK_STRIDE * CTX_NSBUF);
    if (st == MMC_OK) {
        const hipError_t e = hipStreamCreateWithFlags(&c->srv.stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            mmc_set_error("hipStreamCreateWithFlags failed: %s", hipGetErrorString(e));
            st = MMC_ERR_HIP;
        }
    }
    if (const char *e = getenv("MMC_CTX_SERVER"))
        c->server_mode = atoi(e) ? -1 : 0;
    if (st != MMC_OK) {
        mmc_ctx_destroy(c);
        return st;
    }
    *out = c;
    return MMC_OK;
}

static void study_release(mmc_ctx *ctx); // fp32 study buffers, end of this file
static int32_t ctx_server_stop(mmc_ctx *ctx);

extern "C" int32_t mmc_ctx_destroy(mmc_ctx *ctx)
{
    if (!ctx)
        return MMC_OK;
    (void)hipSetDevice(ctx->sys.device);
    (void)ctx_server_stop(ctx);
    if (ctx->sys.stream)
        (void)hipStreamSynchronize(ctx->sys.stream);
    for (void *p : { (void *)ctx->h_move, (void *)ctx->h_parts, (void *)ctx->srv.h_cmd,
                     (void *)ctx->srv.h_out, (void *)ctx->srv.h_state, (void *)ctx->srv.h_smir })
        if (p)
            (void)hipHostFree(p);
    if (ctx->srv.stream)
        (void)hipStreamDestroy(ctx->srv.stream);
    if (ctx->srv.bar_cmd)
        (void)hipFree(ctx->srv.bar_cmd);
    study_release(ctx);
    ctx->sys.release();
    delete ctx;
    return MMC_OK;
}

// =================================================================================================
// the persistent server: start / stop / one command
// =================================================================================================
// The command block as the server sees it: h_cmd itself (pinned), or its copy in BAR memory.  The
// server accepts a block when head and tags agree and trusts that a line whose tag is current holds
// current data (mmc_ctxsrv.hpp).  Ordinary stores to pinned memory become visible in program order;
// stores to BAR memory are write-combining, and a write-combining buffer that is evicted part-way
// through a line may deliver a tag before that line's data.  So on the BAR path the order is made
// explicit: every data word, a fence that drains the write-combining buffers, then the eight tags
// and the head, and a second fence that sends those on their way.
template <class Srv> static void ctx_cmd_publish(Srv &sv, bool head_only = false)
{
    if (!sv.bar_cmd)
        return;
    volatile unsigned long long *dst = sv.bar_cmd;
    const int last = head_only ? 0 : 7;
    for (int l = last; l >= 0; l--)
        for (int q = 6; q >= (l == 0 ? 1 : 0); q--) // neither the tag (word 7) nor the head (word 0 of line 0)
            dst[8 * l + q] = sv.h_cmd[8 * l + q];
    mmc_bar_flush();
    for (int l = last; l >= 0; l--)
        dst[8 * l + 7] = sv.h_cmd[8 * l + 7];
    dst[CS_W_HEAD] = sv.h_cmd[CS_W_HEAD];
    mmc_bar_flush();
}

static int32_t ctx_server_stop(mmc_ctx *ctx)
{
    auto &sv = ctx->srv;
    if (!sv.alive)
        return MMC_OK;
    __atomic_store_n(&sv.h_cmd[CS_W_HEAD], (unsigned long long)CS_QUIT, __ATOMIC_RELEASE);
    ctx_cmd_publish(sv, true);
    sv.alive = false;
    MMC_HIP(hipStreamSynchronize(sv.stream));
#ifdef CS_PROFILE
    for (int w = 0; w < sv.wpg; w++) {
        const int32_t *t = sv.h_state + 16 + 8 * w;
        if (t[3] > 0)
            fprintf(stderr, "ctx server wave %d: wait %.2f us, barrier %.2f, unit %.2f (per evaluation, %d)\n", w,
                    t[0] * 0.01 / t[3], t[1] * 0.01 / t[3], t[2] * 0.01 / t[3], t[3]);
    }
#endif
    return MMC_OK;
}

// Can the server answer for these cutoffs?  Homogeneous 3-site molecules with records, an erfc
// table that covers the cutoff, RecipMove's preconditions (ewalds.jl:740-743).
static bool ctx_server_applies(const mmc_ctx *ctx, double qq_rcut)
{
    const DeviceSystem &s = ctx->sys;
    return ctx->server_mode != 0 && s.uploaded && s.ewald_ready && s.fast_table_ok(qq_rcut) && s.n_mol <= MMC_WAVE_MAX_MOL
           && s.k_sq_max == 27 && s.nk == 5 && s.n_mol < (1 << 27);
}

static int32_t ctx_server_start(mmc_ctx *ctx, double lj_rcut, double qq_rcut, double ovr)
{
    auto &sv = ctx->srv;
    DeviceSystem &s = ctx->sys;
    if (sv.alive && sv.lj_rcut == lj_rcut && sv.qq_rcut == qq_rcut && sv.ovr == ovr
        && sv.kappa == s.bv.kappa && sv.box == s.box) {
        // a server that has not been spoken to for a while may be about to give up (CS_IDLE_TICKS):
        // replace it rather than race its timeout
        if (std::chrono::steady_clock::now() - sv.last_post < std::chrono::milliseconds(300))
            return MMC_OK;
    }
    MMC_TRY(ctx_server_stop(ctx));
    MMC_HIP(hipStreamSynchronize(s.stream)); // launches of the context's own stream come first
    int G = 1, wpg = SRV_WAVES;
    if (const char *e = getenv("MMC_CTX_WGS")) G = atoi(e);
    if (const char *e = getenv("MMC_CTX_WAVES")) wpg = atoi(e);
    if (wpg < 1) wpg = 1;
    if (wpg > SRV_WAVES) wpg = SRV_WAVES;
    if (G < 1) G = 1;
    if (G * wpg > MMC_MAX_PARTS) G = MMC_MAX_PARTS / wpg;
    if (G * wpg < 2) wpg = 2;
    // the latency form when every pair part's molecule range fits a wave's resident storage:
    // four workgroups of four waves (fewer if that is enough)
    int latG = 4;
    if (const char *e = getenv("MMC_CTX_LAT")) latG = atoi(e);
    while (latG >= 1 && !lat_applies(LAT_WAVES * latG, (int)s.n_mol, (int)s.nkvecs))
        latG--;
    if (latG < 1 && !getenv("MMC_CTX_LAT")) { // a large system: as many workgroups as it takes (10 000 molecules: 21)
        latG = (int)(((s.n_mol + LAT_MAXMOL - 1) / LAT_MAXMOL + 3 + LAT_WAVES - 1) / LAT_WAVES);
        while (latG <= MMC_CTX_MAX_WGS && !lat_applies(LAT_WAVES * latG, (int)s.n_mol, (int)s.nkvecs))
            latG++;
        if (latG > MMC_CTX_MAX_WGS)
            latG = 0;
    }
    sv.lat = latG >= 1 && !getenv("MMC_CTX_WGS");
    if (sv.lat) {
        G = latG; wpg = LAT_WAVES;
    }
    sv.G = G; sv.wpg = wpg; sv.P = sv.lat ? G : G * wpg;
    sv.look_ahead = sv.lat && s.n_mol > 2 && !(getenv("MMC_CTX_LOOKAHEAD") && !atoi(getenv("MMC_CTX_LOOKAHEAD")));
    sv.lj_rcut = lj_rcut; sv.qq_rcut = qq_rcut; sv.ovr = ovr; sv.kappa = s.bv.kappa; sv.box = s.box;
    memset(sv.h_state, 0, 512);
    // the command word in memory is the last one posted (or a quit): the new launch must not take
    // it for its first command unless the host posts it again
    __atomic_store_n(&sv.h_cmd[CS_W_HEAD], 0ULL, __ATOMIC_RELEASE);
    ctx_cmd_publish(sv, true);
    CtxSrvArgs sa;
    sa.cmd = sv.bar_cmd ? sv.bar_cmd : sv.d_cmd;
    sa.s_mirror = sv.d_smir;
    sa.state = sv.d_state;
    sa.seq0 = sv.seq + 1;
    const PairParams pp = mmc_pair_params(lj_rcut, qq_rcut, 0.0, ovr, s.bv.kappa, false);
    if (sv.lat)
        k_ctx_server_lat<<<(unsigned)(sv.look_ahead ? 2 * G : G), LAT_WAVES * 64, 0, sv.stream>>>(
            s.bv, s.rec, s.qq_tab, s.kpack, s.fc, sv.d_out, LAT_WAVES * G, pp, sa);
    else
        k_ctx_server<<<(unsigned)G, wpg * 64, 0, sv.stream>>>(s.bv, s.rec, s.qq_tab, s.kpack, s.fc,
                                                              sv.d_out, sv.P, pp, sa);
    MMC_HIP(hipGetLastError());
    sv.alive = true;
    sv.n_launches++;
    sv.last_post = std::chrono::steady_clock::now();
    return MMC_OK;
}

// logical word L of the command block (mmc_ctxsrv.hpp: every eighth physical word is a tag)
#define CMDW(c, L) ((c)[CS_PHYS(L)])

// Post one command (words 1.. are filled by the caller in sv.h_cmd) and wait for the parts.
static int32_t ctx_server_exec(mmc_ctx *ctx, unsigned flags, CtxEval *ev)
{
    auto &sv = ctx->srv;
    DeviceSystem &s = ctx->sys;
    const int P = sv.P;
    for (int attempt = 0; attempt < 3; attempt++) {
        if (!sv.alive)
            MMC_TRY(ctx_server_start(ctx, sv.lj_rcut, sv.qq_rcut, sv.ovr));
        const unsigned long long seq = ++sv.seq; // (a replacement server starts at the next number)
        const unsigned stamp = (++sv.stamp) & MMC_STAMP_MASK;
        CMDW(sv.h_cmd, CS_W_SBUF) = (CMDW(sv.h_cmd, CS_W_SBUF) & 0xffffffffULL) | ((unsigned long long)stamp << 32);
        std::atomic_thread_fence(std::memory_order_release);
        for (int t = 7; t < 64; t += 8) // the tags close their lines, the head the block
            __atomic_store_n(&sv.h_cmd[t], seq, __ATOMIC_RELEASE);
        __atomic_store_n(&sv.h_cmd[CS_W_HEAD], (seq << 16) | (flags & 0xffffu), __ATOMIC_RELEASE);
        ctx_cmd_publish(sv);
        const auto t_post = std::chrono::steady_clock::now();
        sv.last_post = t_post;
        sv.n_cmds++;
        PartOut parts[2 * MMC_MAX_PARTS];
        bool ok = true;
        // records to wait for: P results; the latency form adds the S-mirror sums of the
        // workgroups that hold reciprocal waves (out[CS_OUT_SSUM(G, g)]) when the command has that part
        int idx[2 * MMC_MAX_PARTS], n_idx = 0;
        for (int q = 0; q < P; q++)
            idx[n_idx++] = q;
        if (sv.lat && (flags & CS_RECIP)) {
            const LatPlan pl = lat_plan(LAT_WAVES * sv.G, (int)s.n_mol, (int)s.nkvecs);
            for (int g = 0; g < sv.G; g++)
                if ((g + 1) * LAT_WAVES > pl.np)
                    idx[n_idx++] = CS_OUT_SSUM(sv.G, g);
        }
        for (int q = 0; q < n_idx && ok; q++) {
            const PartOut *src = &sv.h_out[idx[q]];
            for (unsigned spins = 1;; spins++) {
                if (part_stamp_of(*(const volatile int32_t *)&src->ovl[1]) == (stamp & MMC_STAMP_MASK)) {
                    std::atomic_thread_fence(std::memory_order_acquire);
                    if (part_copy_checked(src, stamp, &parts[q]))
                        break;
                }
                if ((spins & 0x3ff) == 0) {
                    const auto dt = std::chrono::steady_clock::now() - t_post;
                    if (__atomic_load_n(sv.h_state, __ATOMIC_ACQUIRE)
                        || dt > std::chrono::milliseconds(attempt == 0 ? 50 : 2000)) {
                        ok = false; // a workgroup gave up, or the reply is late: replace the server
                        break;
                    }
                }
            }
        }
        if (ok) {
            memset(ev, 0, sizeof(*ev));
            if (sv.lat) { // one record per workgroup, every term summed over them in order
                for (int q = 0; q < P; q++) {
                    for (int st = 0; st < 2; st++) {
                        ev->lj_pot[st] += parts[q].lj_pot[st];
                        ev->lj_vir[st] += parts[q].lj_vir[st];
                        ev->qq_pot[st] += parts[q].qq_pot[st];
                        ev->ovl[st] |= parts[q].ovl[st] & 1;
                    }
                    ev->recip += parts[q].recip;
                }
                for (int q = P; q < n_idx; q++) {
                    unsigned long long ss;
                    memcpy(&ss, &parts[q].lj_pot[0], 8);
                    ev->s_sum += ss;
                }
                return MMC_OK;
            }
            for (int q = 0; q < P - 1; q++)
                for (int st = 0; st < 2; st++) {
                    ev->lj_pot[st] += parts[q].lj_pot[st];
                    ev->lj_vir[st] += parts[q].lj_vir[st];
                    ev->qq_pot[st] += parts[q].qq_pot[st];
                    ev->ovl[st] |= parts[q].ovl[st] & 1;
                }
            ev->recip = parts[P - 1].recip;
            memcpy(&ev->s_sum, &parts[P - 1].lj_pot[0], 8);
            return MMC_OK;
        }
        // every command is idempotent (absolute coordinates, S_dst = S_base + dS): stop whatever is
        // left of the server, start a new one and post the same command again
        sv.n_retries++;
        MMC_TRY(ctx_server_stop(ctx));
        const hipError_t e = hipGetLastError();
        MMC_REQUIRE(e == hipSuccess, MMC_ERR_HIP, "the context server failed: %s", hipGetErrorString(e));
    }
    (void)s;
    mmc_set_error("the context server did not answer (3 attempts)");
    return MMC_ERR_HIP;
}

// =================================================================================================
// mirror, stale molecules
// =================================================================================================
static void ctx_mirror_catch_up(mmc_ctx *ctx);

static void ctx_mirror_reset(mmc_ctx *ctx, const double *com, const double *coords)
{
    DeviceSystem &s = ctx->sys;
    if (!(com && coords))
        ctx_mirror_catch_up(ctx); // (what is not replaced must be current)
    else
        ctx->mirror_scale.clear();
    if (com)
        ctx->m_com.assign(com, com + 3 * s.n_mol);
    if (coords)
        ctx->m_at.assign(coords, coords + 3 * s.n_atoms);
    ctx->dirty.clear();
    ctx->version++;
    ctx->ec.valid = false;
    ctx->rc.valid = false;
    ctx->prev_trial.valid = false;
}

// Volume moves rescale the device's coordinates (k_rescale); the host mirror follows with the same
// arithmetic -- nw = old * f, atoms += nw - old, bit for bit the device's -- but only when it is
// next looked at (a 10 000-molecule mirror costs ~40 us per factor).
static void ctx_mirror_catch_up(mmc_ctx *ctx)
{
    if (ctx->mirror_scale.empty())
        return;
    DeviceSystem &s = ctx->sys;
    for (const double f : ctx->mirror_scale)
        for (int64_t j = 0; j < s.n_mol; j++) {
            double *c = &ctx->m_com[3 * (size_t)j];
            double *at = &ctx->m_at[3 * (size_t)s.h_first0[j]];
            for (int k = 0; k < 3; k++) {
                const double old = c[k], nw = old * f, d = nw - old;
                c[k] = nw;
                for (int a = 0; a < s.h_cnt[j]; a++)
                    at[3 * a + k] += d;
            }
        }
    ctx->mirror_scale.clear();
}

// The caller's molecule i (1-based): com[3], atoms[3 * na].  Returns true if it changed.
static bool ctx_sync_mol(mmc_ctx *ctx, int64_t i, const double *com, const double *atoms)
{
    DeviceSystem &s = ctx->sys;
    ctx_mirror_catch_up(ctx);
    const int32_t m = (int32_t)(i - 1), fa = s.h_first0[m], na = s.h_cnt[m];
    double *mc = &ctx->m_com[3 * (size_t)m], *ma = &ctx->m_at[3 * (size_t)fa];
    if (!memcmp(mc, com, 24) && !memcmp(ma, atoms, 24 * (size_t)na))
        return false;
    size_t k = 0;
    for (; k < ctx->dirty.size(); k++)
        if (ctx->dirty[k].mol == m)
            break;
    if (k == ctx->dirty.size()) { // the device holds what the mirror held
        CtxDirty d;
        d.mol = m;
        d.has_dev_rec = na == 3;
        if (d.has_dev_rec) {
            memcpy(d.dev_rec, ma, 72);
            memcpy(d.dev_rec + 9, mc, 24);
        }
        ctx->dirty.push_back(d);
    }
    memcpy(mc, com, 24);
    memcpy(ma, atoms, 24 * (size_t)na);
    for (int a = 0; a < na; a++) { // the caller's coordinates: keep DeviceSystem::r_mol_max a bound
        const double dx = atoms[3 * a] - com[0], dy = atoms[3 * a + 1] - com[1], dz = atoms[3 * a + 2] - com[2];
        s.r_mol_max = std::max(s.r_mol_max, std::sqrt(dx * dx + dy * dy + dz * dz));
    }
    const CtxDirty &d = ctx->dirty[k];
    if (d.has_dev_rec && !memcmp(d.dev_rec, ma, 72) && !memcmp(d.dev_rec + 9, mc, 24))
        ctx->dirty.erase(ctx->dirty.begin() + (long)k); // back to what the device holds
    ctx->version++;
    return true;
}

// Bring the device in step with the mirror through ordinary launches (everything that is not a
// server command starts with this, after the server has been stopped).
static int32_t ctx_flush_dirty(mmc_ctx *ctx)
{
    DeviceSystem &s = ctx->sys;
    for (const CtxDirty &d : ctx->dirty) {
        SetMolArgs a;
        a.r = 0; a.i0 = d.mol; a.na = s.h_cnt[d.mol]; a._pad = 0;
        for (int k = 0; k < 3; k++)
            a.com[k] = ctx->m_com[3 * (size_t)d.mol + k];
        const double *ma = &ctx->m_at[3 * (size_t)s.h_first0[d.mol]];
        for (int t = 0; t < a.na; t++)
            for (int k = 0; k < 3; k++)
                a.at[t][k] = ma[3 * t + k];
        k_set_molecule<<<1, 64, 0, s.stream>>>(s.bv, a, s.rec);
        s.comq_epoch++;
    }
    if (!ctx->dirty.empty())
        MMC_HIP(hipGetLastError());
    ctx->dirty.clear();
    return MMC_OK;
}

// Before anything that launches on the context's stream or copies device memory.
static int32_t ctx_quiesce(mmc_ctx *ctx)
{
    MMC_TRY(ctx_server_stop(ctx));
    return ctx_flush_dirty(ctx);
}

// ---- structure-factor buffers ---------------------------------------------------------------------
static int ctx_free_sbuf(const mmc_ctx *ctx)
{
    for (int b = 0; b < CTX_NSBUF; b++)
        if (b != ctx->s_old && b != ctx->s_new && !(ctx->rc.valid && (b == ctx->rc.dst || b == ctx->rc.base)))
            return b;
    return -1; // (cannot happen: at most 3 of the 4 are named)
}

static double *ctx_smirror(mmc_ctx *ctx, int b) { return ctx->srv.h_smir + (size_t)b * 2 * MMC_NK_STRIDE; }

static int32_t ctx_pull_sbuf(mmc_ctx *ctx, int b) // device buffer b -> its host mirror
{
    if (ctx->m_valid[b])
        return MMC_OK;
    DeviceSystem &s = ctx->sys;
    MMC_TRY(ctx_quiesce(ctx));
    MMC_TRY(s.sync());
    MMC_HIP(hipMemcpy(ctx_smirror(ctx, b), s.bv.S + (size_t)b * 2 * s.bv.nk_stride,
                      sizeof(double) * 2 * s.nkvecs, hipMemcpyDeviceToHost));
    ctx->m_valid[b] = true;
    return MMC_OK;
}

// The generic kernels know buffers 0 and 1 only (old = 0, new = 1): bring the named buffers there.
static int32_t ctx_normalize_sbufs(mmc_ctx *ctx)
{
    DeviceSystem &s = ctx->sys;
    if (!s.ewald_ready || (ctx->s_old == 0 && (ctx->s_new == 0 || ctx->s_new == 1)))
        return MMC_OK;
    MMC_TRY(ctx_quiesce(ctx));
    const unsigned g = (unsigned)((2 * s.nkvecs + 255) / 256);
    const int o = ctx->s_old, n = ctx->s_new;
    if (n != o && n == 0) { // sumQExpNew sits where sumQExpOld must go: through a third buffer
        const int t = o == 2 ? 3 : 2;
        k_copy_s<<<g, 256, 0, s.stream>>>(s.bv, t, 0);
        k_copy_s<<<g, 256, 0, s.stream>>>(s.bv, 0, o);
        k_copy_s<<<g, 256, 0, s.stream>>>(s.bv, 1, t);
        ctx->m_valid[t] = ctx->m_valid[0] = ctx->m_valid[1] = false;
    } else {
        if (o != 0) {
            k_copy_s<<<g, 256, 0, s.stream>>>(s.bv, 0, o);
            ctx->m_valid[0] = false;
        }
        if (n != o && n != 1) {
            k_copy_s<<<g, 256, 0, s.stream>>>(s.bv, 1, n);
            ctx->m_valid[1] = false;
        }
    }
    MMC_HIP(hipGetLastError());
    ctx->s_old = 0;
    ctx->s_new = n != o ? 1 : 0;
    ctx->rc.valid = false;
    return MMC_OK;
}

extern "C" int32_t mmc_ctx_synchronize(mmc_ctx *ctx)
{
    CTX_CHECK(ctx);
    MMC_TRY(ctx_quiesce(ctx));
    return ctx->sys.sync();
}

extern "C" int32_t mmc_upload_system(mmc_ctx *ctx, int64_t n_mol, int64_t n_atoms,
                                     const double *com, const int64_t *first_atom,
                                     const int64_t *last_atom, const double *coords,
                                     const int64_t *atype, const double *charge, int64_t n_types,
                                     const double *eps, const double *sig, double box)
{
    CTX_CHECK(ctx);
    CTX_NO_VOLUME_TRIAL(ctx);
    MMC_TRY(ctx->sys.upload(n_mol, n_atoms, com, first_atom, last_atom, coords, atype, charge,
                            n_types, eps, sig, box));
    // one chain: split the molecule range over several workgroups to cut the latency of a move
    int np = (int)((n_mol + 127) / 128);
    ctx->n_parts = 1 + (np < 1 ? 1 : np > 63 ? 63 : np);
    ctx_mirror_reset(ctx, com, coords);
    return MMC_OK;
}

extern "C" int32_t mmc_set_molecule(mmc_ctx *ctx, int64_t i, const double *com,
                                    const double *atoms)
{
    CTX_CHECK(ctx);
    CTX_NO_VOLUME_TRIAL(ctx);
    CTX_MOL(ctx, i);
    MMC_REQUIRE(com && atoms, MMC_ERR_ARG, "NULL array argument");
    MMC_REQUIRE(ctx->sys.h_cnt[i - 1] <= MMC_MAX_ATOMS, MMC_ERR_UNSUPPORTED,
                "molecule %lld has %d atoms; a moved molecule may have at most %d",
                (long long)i, ctx->sys.h_cnt[i - 1], MMC_MAX_ATOMS);
    (void)ctx_sync_mol(ctx, i, com, atoms); // travels with the next evaluation
    return MMC_OK;
}

extern "C" int32_t mmc_update_system(mmc_ctx *ctx, const double *com, const double *coords)
{
    CTX_CHECK(ctx);
    CTX_NO_VOLUME_TRIAL(ctx);
    MMC_TRY(ctx_server_stop(ctx));
    ctx->dirty.clear(); // everything is re-sent
    MMC_TRY(ctx->sys.set_replica(0, com, coords));
    ctx_mirror_reset(ctx, com, coords);
    return MMC_OK;
}

extern "C" int32_t mmc_volume_change(mmc_ctx *ctx, double new_box, double new_kappa)
{
    CTX_CHECK(ctx);
    MMC_REQUIRE(!ctx->trial_outstanding, MMC_ERR_STATE,
                "trial move not settled: call mmc_accept_move or mmc_reject_move first");
    MMC_REQUIRE(!ctx->vol.outstanding, MMC_ERR_STATE,
                "volume move not settled: call mmc_volume_accept or mmc_volume_reject first");
    MMC_TRY(ctx_quiesce(ctx));
    const double f = new_box / ctx->sys.box; // k_rescale's factor
    MMC_TRY(ctx->sys.volume_change(new_box, new_kappa));
    ctx->mirror_scale.push_back(f); // the mirror follows when it is next looked at
    ctx->version++;
    ctx->ec.valid = false;
    ctx->rc.valid = false;
    ctx->prev_trial.valid = false;
    ctx->s_old = ctx->s_new = 0; // zeroed sumQExp arrays (ewalds.jl:98-99)
    for (bool &v : ctx->m_valid) v = false;
    return MMC_OK;
}

// An NPT volume move without a host round trip (the reference's only statement of the move is the
// docstring Ewald/volumeChange.jl:59-147).  Trial: everything the move rewrites -- coordinates in
// their three layouts, fixed-point centres of mass, S(k), k-vectors, erfc table -- is copied
// aside ON THE DEVICE (one launch), then the system is rescaled, the tables rebuilt for
// kappa = alpha / L_new and the total energy evaluated at the new volume (:91-111).  Accept
// (:132-147): nothing.  Reject: the copy back (one launch).
extern "C" int32_t mmc_volume_trial(mmc_ctx *ctx, double new_box, double new_kappa, double lj_rcut,
                                    double qq_rcut, mmc_totals *tot)
{
    CTX_CHECK(ctx);
    MMC_REQUIRE(tot, MMC_ERR_ARG, "NULL out pointer");
    MMC_REQUIRE(!ctx->trial_outstanding && !ctx->vol.outstanding, MMC_ERR_STATE,
                "a trial move is not settled");
    MMC_TRY(ctx_quiesce(ctx));
    MMC_TRY(ctx->sys.snapshot_take());
    ctx->vol.n_scale = ctx->mirror_scale.size();
    ctx->vol.s_old = ctx->s_old; ctx->vol.s_new = ctx->s_new;
    for (int b = 0; b < CTX_NSBUF; b++) ctx->vol.m_valid[b] = ctx->m_valid[b];
    int32_t st = mmc_volume_change(ctx, new_box, new_kappa);
    if (st == MMC_OK)
        st = mmc_potential_ewald(ctx, lj_rcut, qq_rcut, tot);
    if (st != MMC_OK) { // leave the context as it was
        (void)ctx->sys.snapshot_restore();
        ctx->mirror_scale.resize(ctx->vol.n_scale);
        ctx->s_old = ctx->vol.s_old; ctx->s_new = ctx->vol.s_new;
        for (int b = 0; b < CTX_NSBUF; b++) ctx->m_valid[b] = ctx->vol.m_valid[b];
        ctx->version++;
        return st;
    }
    ctx->vol.outstanding = true;
    return MMC_OK;
}

extern "C" int32_t mmc_volume_accept(mmc_ctx *ctx)
{
    CTX_CHECK(ctx);
    MMC_REQUIRE(ctx->vol.outstanding, MMC_ERR_STATE, "no volume move outstanding");
    ctx->vol.outstanding = false;
    ctx->sys.snap.valid = false;
    return MMC_OK;
}

extern "C" int32_t mmc_volume_reject(mmc_ctx *ctx)
{
    CTX_CHECK(ctx);
    MMC_REQUIRE(ctx->vol.outstanding, MMC_ERR_STATE, "no volume move outstanding");
    MMC_TRY(ctx_quiesce(ctx));
    MMC_TRY(ctx->sys.snapshot_restore()); // ordered before whatever the stream runs next
    ctx->mirror_scale.resize(ctx->vol.n_scale);
    ctx->s_old = ctx->vol.s_old; ctx->s_new = ctx->vol.s_new;
    for (int b = 0; b < CTX_NSBUF; b++) ctx->m_valid[b] = ctx->vol.m_valid[b];
    ctx->version++;
    ctx->ec.valid = false;
    ctx->rc.valid = false;
    ctx->vol.outstanding = false;
    return MMC_OK;
}

extern "C" int32_t mmc_download_system(mmc_ctx *ctx, double *com, double *coords)
{
    CTX_CHECK(ctx);
    MMC_TRY(ctx_quiesce(ctx));
    return ctx->sys.get_replica(0, com, coords);
}

extern "C" int32_t mmc_prepare_ewald(mmc_ctx *ctx, double kappa, int64_t nk, int64_t k_sq_max,
                                     double box, double factor, int64_t *nkvecs)
{
    CTX_CHECK(ctx);
    CTX_NO_VOLUME_TRIAL(ctx);
    MMC_TRY(ctx_quiesce(ctx));
    MMC_TRY(ctx->sys.prepare_ewald(kappa, nk, k_sq_max, box, factor, nkvecs));
    ctx->s_old = ctx->s_new = 0; // zeroed sumQExp arrays (ewalds.jl:98-99)
    for (bool &v : ctx->m_valid) v = false;
    ctx->ec.valid = false;
    ctx->rc.valid = false;
    return MMC_OK;
}

extern "C" int32_t mmc_get_kvectors(mmc_ctx *ctx, int32_t *kxyz, double *cfac)
{
    CTX_CHECK(ctx);
    DeviceSystem &s = ctx->sys;
    MMC_REQUIRE(s.ewald_ready, MMC_ERR_STATE, "PrepareEwaldVariables has not run");
    MMC_TRY(s.sync());
    if (kxyz)
        MMC_HIP(hipMemcpy(kxyz, s.bv.kxyz, sizeof(int32_t) * 3 * s.nkvecs, hipMemcpyDeviceToHost));
    if (cfac)
        MMC_HIP(hipMemcpy(cfac, s.bv.cfac, sizeof(double) * s.nkvecs, hipMemcpyDeviceToHost));
    return MMC_OK;
}

extern "C" int32_t mmc_get_sumqexp(mmc_ctx *ctx, double *sum_old, double *sum_new)
{
    CTX_CHECK(ctx);
    DeviceSystem &s = ctx->sys;
    MMC_REQUIRE(s.ewald_ready, MMC_ERR_STATE, "PrepareEwaldVariables has not run");
    if (sum_old) {
        MMC_TRY(ctx_pull_sbuf(ctx, ctx->s_old));
        memcpy(sum_old, ctx_smirror(ctx, ctx->s_old), sizeof(double) * 2 * s.nkvecs);
    }
    if (sum_new) {
        MMC_TRY(ctx_pull_sbuf(ctx, ctx->s_new));
        memcpy(sum_new, ctx_smirror(ctx, ctx->s_new), sizeof(double) * 2 * s.nkvecs);
    }
    return MMC_OK;
}

extern "C" int32_t mmc_set_sumqexp(mmc_ctx *ctx, const double *sum_old, const double *sum_new)
{
    CTX_CHECK(ctx);
    CTX_NO_VOLUME_TRIAL(ctx);
    DeviceSystem &s = ctx->sys;
    MMC_REQUIRE(s.ewald_ready, MMC_ERR_STATE, "PrepareEwaldVariables has not run");
    MMC_TRY(ctx_normalize_sbufs(ctx)); // an array that is not given keeps its content, in buffer 0 / 1
    MMC_TRY(ctx_quiesce(ctx));
    MMC_TRY(s.sync());
    const size_t bytes = sizeof(double) * 2 * s.nkvecs;
    if (ctx->s_new == ctx->s_old && (sum_old || sum_new)) { // the two arrays part ways
        const unsigned g = (unsigned)((2 * s.nkvecs + 255) / 256);
        k_copy_s<<<g, 256, 0, s.stream>>>(s.bv, 1, 0);
        MMC_HIP(hipGetLastError());
        MMC_TRY(s.sync());
        ctx->m_valid[1] = false;
        ctx->s_new = 1;
    }
    if (sum_old) {
        MMC_HIP(hipMemcpy(s.bv.S, sum_old, bytes, hipMemcpyHostToDevice));
        memcpy(ctx_smirror(ctx, 0), sum_old, bytes);
        ctx->m_valid[0] = true;
    }
    if (sum_new) {
        MMC_HIP(hipMemcpy(s.bv.S + 2 * s.bv.nk_stride, sum_new, bytes, hipMemcpyHostToDevice));
        memcpy(ctx_smirror(ctx, 1), sum_new, bytes);
        ctx->m_valid[1] = true;
    }
    ctx->rc.valid = false;
    return MMC_OK;
}

// =================================================================================================
// per-molecule evaluation: LJ and real-space Coulomb together, cached
// =================================================================================================
static void ctx_fill_cmd_mol(mmc_ctx *ctx, int32_t m /* 0-based */, const double *rec_new,
                             const double *rec_old)
{
    unsigned long long *c = ctx->srv.h_cmd;
    MoveRec mv;
    memset(&mv, 0, sizeof(mv));
    mv.mol = m + 1;
    memcpy(mv.atoms_new, rec_new, 72);
    memcpy(mv.com_new, rec_new + 9, 24);
    if (rec_old) {
        memcpy(mv.atoms_old, rec_old, 72);
        memcpy(mv.com_old, rec_old + 9, 24);
    }
    const unsigned long long *mw = reinterpret_cast<const unsigned long long *>(&mv);
    for (int q = 0; q < MV_Q_NEW; q++)
        CMDW(c, CS_W_MV + q) = mw[q];
}

// stale molecules of the mirror -> pending slots of the command; more than CS_MAX_PEND are sent
// ahead in commands of their own.  Leaves n_pend in the command.
static int32_t ctx_cmd_pending(mmc_ctx *ctx)
{
    DeviceSystem &s = ctx->sys;
    unsigned long long *c = ctx->srv.h_cmd;
    size_t k = 0;
    for (;;) {
        int n = 0;
        for (; k < ctx->dirty.size() && n < CS_MAX_PEND; k++, n++) {
            const int32_t m = ctx->dirty[k].mol;
            unsigned long long &pmw = CMDW(c, CS_W_PMOL);
            pmw = n == 0 ? (unsigned long long)(uint32_t)m
                         : (pmw & 0xffffffffULL) | ((unsigned long long)(uint32_t)m << 32);
            const unsigned long long *at = reinterpret_cast<const unsigned long long *>(
                                         &ctx->m_at[3 * (size_t)s.h_first0[m]]),
                                     *cm = reinterpret_cast<const unsigned long long *>(&ctx->m_com[3 * (size_t)m]);
            for (int q = 0; q < 9; q++)
                CMDW(c, CS_W_PREC + 12 * n + q) = at[q];
            for (int q = 0; q < 3; q++)
                CMDW(c, CS_W_PREC + 12 * n + 9 + q) = cm[q];
        }
        CMDW(c, CS_W_MOL) = (CMDW(c, CS_W_MOL) & 0xffffffffULL) | ((unsigned long long)(uint32_t)n << 32);
        if (k >= ctx->dirty.size())
            break;
        CtxEval ev; // an update-only command
        MMC_TRY(ctx_server_exec(ctx, 0u, &ev));
    }
    return MMC_OK;
}

static int32_t ctx_verify_smirror(mmc_ctx *ctx, int b, unsigned long long want)
{
    const double *m = ctx_smirror(ctx, b);
    const int64_t n = ctx->sys.nkvecs;
    for (int tries = 0; tries < 100000; tries++) {
        unsigned long long sum = 0;
        for (int64_t k = 0; k < n; k++) {
            unsigned long long re, im;
            re = ((const volatile unsigned long long *)m)[2 * k];
            im = ((const volatile unsigned long long *)m)[2 * k + 1];
            sum += re + 3ULL * im;
        }
        if (sum == want)
            return MMC_OK;
        std::atomic_thread_fence(std::memory_order_acquire);
    }
    mmc_set_error("the structure factor the server sent to the host never became consistent");
    return MMC_ERR_HIP;
}

// Evaluate molecule i (1-based) at the mirror's coordinates.  Fills ctx->ec.
static int32_t ctx_eval_mol(mmc_ctx *ctx, int64_t i, double lj_rcut, double qq_rcut, double ovr,
                            bool want_lj, bool want_qq)
{
    DeviceSystem &s = ctx->sys;
    auto &ec = ctx->ec;
    if (!want_lj) lj_rcut = ctx->last_lj_rcut > 0 ? ctx->last_lj_rcut : qq_rcut;
    if (!want_qq) qq_rcut = ctx->last_qq_rcut > 0 ? ctx->last_qq_rcut : lj_rcut;
    if (want_lj) ctx->last_lj_rcut = lj_rcut;
    if (want_qq) ctx->last_qq_rcut = qq_rcut;
    if (ec.valid && ec.mol == i && ec.version == ctx->version && (!want_lj || (ec.has_lj && ec.lj_rcut == lj_rcut))
        && (!want_qq || (ec.has_qq && ec.qq_rcut == qq_rcut && ec.ovr == ovr))) {
        ctx->n_cache_hits++;
        return MMC_OK;
    }
    const int32_t m = (int32_t)(i - 1);
    MMC_REQUIRE(s.h_cnt[m] <= MMC_MAX_ATOMS, MMC_ERR_UNSUPPORTED,
                "molecule %lld has %d atoms; the chosen molecule may have at most %d",
                (long long)i, s.h_cnt[m], MMC_MAX_ATOMS);
    ec.valid = false;
    ctx_mirror_catch_up(ctx);
    // Look-ahead: Loop() sweeps the molecules in order (main.jl:490), so the command that evaluated
    // molecule i - 1 in its moved state also had the server's second set of workgroups evaluate
    // molecule i as the system stood after that command.  If nothing has changed since (the move
    // was accepted), their records are the answer -- the same kernel, the same part plan, the same
    // sums as a command of its own.
    if (ctx->la.posted) {
        auto &la = ctx->la;
        auto &sv = ctx->srv;
        la.posted = false;
        if (la.mol == i && la.version == ctx->version && sv.alive && sv.lat && la.launch == sv.n_launches
            && la.lj_rcut == lj_rcut && la.qq_rcut == qq_rcut && la.ovr == ovr && ctx->dirty.empty()) {
            PartOut parts[MMC_MAX_PARTS];
            bool ok = true;
            const auto t0 = std::chrono::steady_clock::now();
            for (int q = 0; q < sv.G && ok; q++) {
                const PartOut *src = &sv.h_out[CS_OUT_AHEAD(sv.G, q)];
                for (unsigned spins = 1;; spins++) {
                    if (part_stamp_of(*(const volatile int32_t *)&src->ovl[1]) == (la.stamp & MMC_STAMP_MASK)) {
                        std::atomic_thread_fence(std::memory_order_acquire);
                        if (part_copy_checked(src, la.stamp, &parts[q]))
                            break;
                    }
                    if ((spins & 0xff) == 0
                        && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(200)) {
                        ok = false; // not there (yet): ask for it the ordinary way
                        break;
                    }
                }
            }
            if (ok) {
                double lj = 0, vir = 0, qq = 0;
                int ov = 0;
                for (int q = 0; q < sv.G; q++) {
                    lj += parts[q].lj_pot[1]; vir += parts[q].lj_vir[1]; qq += parts[q].qq_pot[1];
                    ov |= parts[q].ovl[1] & 1;
                }
                ec.lj_pot = lj; ec.lj_vir = vir;
                ec.qq_pot = ov ? 0.0 : qq; // ewalds.jl:359-360
                ec.ovl = ov;
                ec.has_lj = ec.has_qq = true;
                ec.valid = true;
                ec.mol = i;
                ec.version = ctx->version;
                ec.lj_rcut = lj_rcut; ec.qq_rcut = qq_rcut; ec.ovr = ovr;
                ctx->n_la_hits++;
                return MMC_OK;
            }
        }
    }
    if (ctx_server_applies(ctx, qq_rcut)) {
        auto &sv = ctx->srv;
        if (!sv.alive || sv.lj_rcut != lj_rcut || sv.qq_rcut != qq_rcut || sv.ovr != ovr
            || sv.kappa != s.bv.kappa || sv.box != s.box
            || std::chrono::steady_clock::now() - sv.last_post > std::chrono::milliseconds(300))
            MMC_TRY(ctx_server_start(ctx, lj_rcut, qq_rcut, ovr));
        unsigned long long *c = sv.h_cmd;
        // the molecule's device copy, if it is stale, is its OLD state: RecipMove comes for free
        const CtxDirty *di = nullptr;
        for (const CtxDirty &d : ctx->dirty)
            if (d.mol == m && d.has_dev_rec)
                di = &d;
        double rec_new[12];
        memcpy(rec_new, &ctx->m_at[9 * (size_t)m], 72);
        memcpy(rec_new + 9, &ctx->m_com[3 * (size_t)m], 24);
        unsigned flags = CS_EVAL;
        int base = 0, dst = 0;
        ctx->rc.valid = false;
        if (di) {
            // which array the caller will pass as sumQExpOld: the two are equal unless a RecipMove
            // is unsettled; then the molecule of that move tells (kept where it went = committed)
            base = ctx->s_old;
            if (ctx->s_new != ctx->s_old && ctx->prev_trial.valid) {
                const int32_t pm = ctx->prev_trial.mol;
                if (!memcmp(ctx->prev_trial.new_rec, &ctx->m_at[9 * (size_t)pm], 72)
                    && !memcmp(ctx->prev_trial.new_rec + 9, &ctx->m_com[3 * (size_t)pm], 24))
                    base = ctx->s_new;
            }
            dst = ctx_free_sbuf(ctx);
            flags |= CS_RECIP;
        }
        CMDW(c, CS_W_MOL) = (unsigned long long)(uint32_t)m;
        CMDW(c, CS_W_SBUF) = (unsigned long long)(uint32_t)(base | (dst << 8));
        ctx_fill_cmd_mol(ctx, m, rec_new, di ? di->dev_rec : nullptr);
        double r_old_keep[9];
        if (di)
            memcpy(r_old_keep, di->dev_rec, 72);
        MMC_TRY(ctx_cmd_pending(ctx));
        // a moved molecule is being evaluated: the next call of a sweep is molecule i + 1 (main.jl:490)
        const int32_t m2 = (m + 1) % (int32_t)s.n_mol;
        const bool look = di && sv.look_ahead && m2 != m;
        if (look) {
            flags |= CS_NEXT;
            CMDW(c, CS_W_MOL) |= (unsigned long long)(uint32_t)m2 << 36; // hi word: n_pend | mol2 << 4
        }
        CtxEval ev;
        MMC_TRY(ctx_server_exec(ctx, flags, &ev));
        ctx->dirty.clear(); // the device holds the mirror now
        if (look) {
            auto &la = ctx->la;
            la.posted = true;
            la.mol = m2 + 1;
            la.version = ctx->version;
            la.stamp = sv.stamp & MMC_STAMP_MASK;
            la.launch = sv.n_launches;
            la.lj_rcut = lj_rcut; la.qq_rcut = qq_rcut; la.ovr = ovr;
            ctx->n_la_posted++;
        }
        if (flags & CS_RECIP) {
            ctx->m_valid[dst] = false;
            MMC_TRY(ctx_verify_smirror(ctx, dst, ev.s_sum));
            ctx->m_valid[dst] = true;
            auto &rc = ctx->rc;
            rc.valid = true;
            memcpy(rc.r_old, r_old_keep, 72);
            memcpy(rc.r_new, rec_new, 72);
            for (int k = 0; k < 3; k++) rc.q[k] = s.h_charge[3 * (size_t)m + k];
            rc.base = base; rc.dst = dst; rc.dE = ev.recip;
            ctx->prev_trial.valid = true;
            ctx->prev_trial.mol = m;
            memcpy(ctx->prev_trial.new_rec, rec_new, 96);
        }
        ec.lj_pot = ev.lj_pot[1]; ec.lj_vir = ev.lj_vir[1];
        ec.qq_pot = ev.ovl[1] ? 0.0 : ev.qq_pot[1]; // ewalds.jl:359-360: `return 0.0, true`
        ec.ovl = ev.ovl[1];
        ec.has_lj = ec.has_qq = true;
    } else {
        // a launch: the generic kernel, both terms at once when an EWALD is there
        MMC_TRY(ctx_quiesce(ctx));
        const bool qq = s.ewald_ready;
        MMC_REQUIRE(qq || !want_qq, MMC_ERR_STATE,
                    "EwaldReal reads ewald.kappa: call PrepareEwaldVariables first");
        const PairParams pp = mmc_pair_params(lj_rcut, qq_rcut, 0.0, ovr, qq ? s.bv.kappa : 0.0, false);
        MMC_TRY(s.mol_energy(m, 1, true, qq, 0, pp, (MolE *)s.d_res, 1));
        MMC_TRY(s.sync());
        MolE r;
        memcpy(&r, s.h_res, sizeof(MolE));
        ec.lj_pot = r.lj_pot; ec.lj_vir = r.lj_vir; ec.qq_pot = r.qq_pot; ec.ovl = r.ovl;
        ec.has_lj = true; ec.has_qq = qq;
        ctx->n_launch_evals++;
    }
    ec.valid = true;
    ec.mol = i;
    ec.version = ctx->version;
    ec.lj_rcut = lj_rcut; ec.qq_rcut = qq_rcut; ec.ovr = ovr;
    return MMC_OK;
}

extern "C" int32_t mmc_lj_poly_du(mmc_ctx *ctx, int64_t i, double r_cut, double *pot,
                                  double *vir)
{
    CTX_CHECK(ctx);
    CTX_NO_VOLUME_TRIAL(ctx);
    CTX_MOL(ctx, i);
    MMC_REQUIRE(pot && vir, MMC_ERR_ARG, "NULL out pointer");
    MMC_TRY(ctx_eval_mol(ctx, i, r_cut, 0.0, ctx->ec.ovr > 0 ? ctx->ec.ovr : 0.5, true, false));
    *pot = ctx->ec.lj_pot * 4;        // energy.jl:289
    *vir = ctx->ec.lj_vir * 24 / 3.0;
    return MMC_OK;
}

extern "C" int32_t mmc_ewald_real(mmc_ctx *ctx, int64_t i, double r_cut, double ovr, double *pot,
                                  int32_t *overlap)
{
    CTX_CHECK(ctx);
    CTX_NO_VOLUME_TRIAL(ctx);
    CTX_MOL(ctx, i);
    MMC_REQUIRE(pot && overlap, MMC_ERR_ARG, "NULL out pointer");
    MMC_REQUIRE(ctx->sys.ewald_ready, MMC_ERR_STATE,
                "EwaldReal reads ewald.kappa: call PrepareEwaldVariables first");
    MMC_TRY(ctx_eval_mol(ctx, i, 0.0, r_cut, ovr, false, true));
    *pot = ctx->ec.qq_pot;
    *overlap = ctx->ec.ovl;
    return MMC_OK;
}

extern "C" int32_t mmc_ewald_short(mmc_ctx *ctx, int64_t i, double qq_rcut, double *e, double *v,
                                   int32_t *overlap)
{
    MMC_REQUIRE(e && v && overlap, MMC_ERR_ARG, "NULL out pointer");
    double realEwald;
    MMC_TRY(mmc_ewald_real(ctx, i, qq_rcut, 0.5, &realEwald, overlap)); // ewalds.jl:904
    realEwald *= ctx->sys.bv.factor;                                    // :905
    *e = realEwald;
    *v = realEwald / 3;                                                 // :907
    return MMC_OK;
}

extern "C" int32_t mmc_coulomb_real(mmc_ctx *ctx, int64_t i, double r_cut, double *pot,
                                    int32_t *overlap)
{
    CTX_CHECK(ctx);
    CTX_NO_VOLUME_TRIAL(ctx);
    CTX_MOL(ctx, i);
    MMC_REQUIRE(pot && overlap, MMC_ERR_ARG, "NULL out pointer");
    MMC_REQUIRE(r_cut == 10.0, MMC_ERR_ASSERT, "AssertionError: r_cut == 10.0 (energy.jl:648)");
    DeviceSystem &s = ctx->sys;
    MMC_REQUIRE(s.h_cnt[i - 1] <= MMC_MAX_ATOMS, MMC_ERR_UNSUPPORTED,
                "molecule %lld has %d atoms; the chosen molecule may have at most %d",
                (long long)i, s.h_cnt[i - 1], MMC_MAX_ATOMS);
    MMC_TRY(ctx_quiesce(ctx));
    const double diameter = r_cut * 0.25 + 5.0; // energy.jl:642
    MMC_TRY(s.mol_energy((int)(i - 1), 1, false, true, 1,
                         mmc_pair_params(r_cut, r_cut, diameter, 1.0, 0.0, true), (MolE *)s.d_res, 1));
    MMC_TRY(s.sync());
    MolE m;
    memcpy(&m, s.h_res, sizeof(MolE));
    *pot = m.qq_pot;
    *overlap = m.ovl;
    return MMC_OK;
}

// ---- the reference's calls with the caller's own arrays ---------------------------------------------
// Loop() has changed at most molecule i and the molecule of the previous call (moved, or restored
// after a rejection: main.jl:527,552,623-624) since the context last looked.
static int32_t ctx_sync_call(mmc_ctx *ctx, int64_t i, const double *com, const double *coords)
{
    DeviceSystem &s = ctx->sys;
    MMC_REQUIRE(com && coords, MMC_ERR_ARG, "NULL array argument");
    const int64_t j = ctx->last_call_mol;
    if (j >= 1 && j <= s.n_mol && j != i)
        (void)ctx_sync_mol(ctx, j, com + 3 * (j - 1), coords + 3 * (size_t)s.h_first0[j - 1]);
    (void)ctx_sync_mol(ctx, i, com + 3 * (i - 1), coords + 3 * (size_t)s.h_first0[i - 1]);
    ctx->last_call_mol = i;
    return MMC_OK;
}

extern "C" int32_t mmc_call_lj_poly_du(mmc_ctx *ctx, int64_t i, const double *com,
                                       const double *coords, double r_cut, double *pot, double *vir)
{
    CTX_CHECK(ctx);
    CTX_NO_VOLUME_TRIAL(ctx);
    CTX_MOL(ctx, i);
    MMC_TRY(ctx_sync_call(ctx, i, com, coords));
    return mmc_lj_poly_du(ctx, i, r_cut, pot, vir);
}

extern "C" int32_t mmc_call_ewald_real(mmc_ctx *ctx, int64_t i, const double *com,
                                       const double *coords, double r_cut, double ovr, double *pot,
                                       int32_t *overlap)
{
    CTX_CHECK(ctx);
    CTX_NO_VOLUME_TRIAL(ctx);
    CTX_MOL(ctx, i);
    MMC_TRY(ctx_sync_call(ctx, i, com, coords));
    return mmc_ewald_real(ctx, i, r_cut, ovr, pot, overlap);
}

extern "C" int32_t mmc_call_ewald_short(mmc_ctx *ctx, int64_t i, const double *com,
                                        const double *coords, double qq_rcut, double *e, double *v,
                                        int32_t *overlap)
{
    CTX_CHECK(ctx);
    CTX_NO_VOLUME_TRIAL(ctx);
    CTX_MOL(ctx, i);
    MMC_TRY(ctx_sync_call(ctx, i, com, coords));
    return mmc_ewald_short(ctx, i, qq_rcut, e, v, overlap);
}

extern "C" int32_t mmc_recip_long(mmc_ctx *ctx, double *energy)
{
    CTX_CHECK(ctx);
    CTX_NO_VOLUME_TRIAL(ctx);
    MMC_REQUIRE(energy, MMC_ERR_ARG, "NULL out pointer");
    MMC_TRY(ctx_quiesce(ctx));
    MMC_TRY(ctx->sys.recip_long_all(energy));
    ctx->s_old = ctx->s_new = 0; // both arrays get `term` (ewalds.jl:600-601): buffers 0 and 1
    for (bool &v : ctx->m_valid) v = false;
    ctx->rc.valid = false;
    return MMC_OK;
}

static int32_t ctx_recip_preconditions(mmc_ctx *ctx, int64_t n)
{
    DeviceSystem &s = ctx->sys;
    MMC_REQUIRE(s.ewald_ready, MMC_ERR_STATE, "PrepareEwaldVariables has not run");
    MMC_REQUIRE(n == 3, MMC_ERR_ASSERT, "AssertionError: n == 3 (ewalds.jl:740)");
    MMC_REQUIRE(s.k_sq_max == 27, MMC_ERR_ASSERT, "AssertionError: k_sq_max == 27 (ewalds.jl:742)");
    MMC_REQUIRE(s.nk == 5, MMC_ERR_ASSERT, "AssertionError: nk == 5 (ewalds.jl:743)");
    return MMC_OK;
}

// RecipMove on the context's named buffers: sumQExpNew += dS in place (ewalds.jl:805-814), the
// energy against sumQExpOld (:817-821).  When the two arrays are equal (Loop's state at :580) the
// sum goes to a free buffer and the old one stays as it is.
static int32_t ctx_recip_move_device(mmc_ctx *ctx, const double *r_old, const double *r_new,
                                     const double *q, double *d_energy /* no factor */)
{
    DeviceSystem &s = ctx->sys;
    auto &rc = ctx->rc;
    if (rc.valid && ctx->s_new == ctx->s_old && rc.base == ctx->s_old && !memcmp(rc.r_old, r_old, 72)
        && !memcmp(rc.r_new, r_new, 72) && !memcmp(rc.q, q, 24)) {
        ctx->n_spec_hits++; // computed with the evaluation of the moved molecule
        ctx->s_new = rc.dst;
        *d_energy = rc.dE;
        rc.valid = false;
        return MMC_OK;
    }
    if (rc.valid)
        ctx->n_spec_miss++;
    rc.valid = false;
    MMC_TRY(ctx_quiesce(ctx));
    RecipMoveArgs a;
    for (int k = 0; k < 9; k++) {
        a.r_old[k] = r_old[k];
        a.r_new[k] = r_new[k];
    }
    for (int k = 0; k < 3; k++)
        a.q[k] = q[k];
    int dst = ctx->s_new;
    if (ctx->s_new == ctx->s_old)
        dst = ctx_free_sbuf(ctx);
    k_recip_move<<<1, MMC_BLOCK, 0, s.stream>>>(s.bv, a, (double *)s.d_res, ctx->s_old, ctx->s_new, dst);
    MMC_HIP(hipGetLastError());
    MMC_TRY(s.sync());
    ctx->s_new = dst;
    ctx->m_valid[dst] = false;
    *d_energy = *(volatile double *)s.h_res;
    return MMC_OK;
}

extern "C" int32_t mmc_recip_move(mmc_ctx *ctx, const double *r_old, const double *r_new,
                                  const double *q, int64_t n, double *d_energy)
{
    CTX_CHECK(ctx);
    CTX_NO_VOLUME_TRIAL(ctx);
    MMC_REQUIRE(r_old && r_new && q && d_energy, MMC_ERR_ARG, "NULL argument");
    MMC_TRY(ctx_recip_preconditions(ctx, n));
    double e;
    MMC_TRY(ctx_recip_move_device(ctx, r_old, r_new, q, &e));
    *d_energy = e * ctx->sys.bv.factor; // ewalds.jl:825
    return MMC_OK;
}

// RecipMove(box, ewalds, r_old, r_new, qq_q) with the caller's ewalds.sumQExpOld / sumQExpNew:
// Loop() rebinds the two arrays to copies between calls (main.jl:621,628), so which device buffer
// each of them is is found by CONTENT, against the pinned host mirrors of the buffers -- two
// comparisons of 5.4 KB on the host, nothing on the device.
extern "C" int32_t mmc_call_recip_move(mmc_ctx *ctx, const double *r_old, const double *r_new,
                                       const double *q, int64_t n, const double *sum_old,
                                       double *sum_new, double *d_energy)
{
    CTX_CHECK(ctx);
    CTX_NO_VOLUME_TRIAL(ctx);
    MMC_REQUIRE(r_old && r_new && q && d_energy && sum_old && sum_new, MMC_ERR_ARG, "NULL argument");
    MMC_TRY(ctx_recip_preconditions(ctx, n));
    DeviceSystem &s = ctx->sys;
    const size_t bytes = sizeof(double) * 2 * s.nkvecs;
    MMC_TRY(ctx_pull_sbuf(ctx, ctx->s_old));
    MMC_TRY(ctx_pull_sbuf(ctx, ctx->s_new));
    const double *mo = ctx_smirror(ctx, ctx->s_old), *mn = ctx_smirror(ctx, ctx->s_new);
    const bool oo = !memcmp(sum_old, mo, bytes), nn = !memcmp(sum_new, mn, bytes);
    if (oo && nn) {
        // the arrays are the ones the context knows
    } else if (!memcmp(sum_old, mn, bytes) && nn) {
        ctx->s_old = ctx->s_new; // ewald.sumQExpOld = copy(sumQExpNew)   main.jl:621
    } else if (oo && !memcmp(sum_new, mo, bytes)) {
        ctx->s_new = ctx->s_old; // ewald.sumQExpNew = copy(sumQExpOld)   main.jl:628
    } else {
        MMC_TRY(mmc_set_sumqexp(ctx, sum_old, sum_new)); // arrays from somewhere else
        if (!memcmp(sum_old, sum_new, bytes))
            ctx->s_new = ctx->s_old = 0;
    }
    double e;
    MMC_TRY(ctx_recip_move_device(ctx, r_old, r_new, q, &e));
    MMC_TRY(ctx_pull_sbuf(ctx, ctx->s_new));
    memcpy(sum_new, ctx_smirror(ctx, ctx->s_new), bytes); // sumQExpNew updated in place (:805-814)
    *d_energy = e * s.bv.factor;                           // ewalds.jl:825
    return MMC_OK;
}

extern "C" int32_t mmc_recip_commit(mmc_ctx *ctx)
{
    CTX_CHECK(ctx);
    CTX_NO_VOLUME_TRIAL(ctx);
    MMC_REQUIRE(ctx->sys.ewald_ready, MMC_ERR_STATE, "PrepareEwaldVariables has not run");
    ctx->s_old = ctx->s_new; // sumQExpOld <- sumQExpNew   main.jl:621 (a renaming, no copy)
    return MMC_OK;
}

extern "C" int32_t mmc_recip_rollback(mmc_ctx *ctx)
{
    CTX_CHECK(ctx);
    CTX_NO_VOLUME_TRIAL(ctx);
    MMC_REQUIRE(ctx->sys.ewald_ready, MMC_ERR_STATE, "PrepareEwaldVariables has not run");
    ctx->s_new = ctx->s_old; // sumQExpNew <- sumQExpOld   main.jl:628
    return MMC_OK;
}

extern "C" int32_t mmc_ewald_self(mmc_ctx *ctx, double *self_energy)
{
    CTX_CHECK(ctx);
    DeviceSystem &s = ctx->sys;
    MMC_REQUIRE(s.uploaded && s.ewald_ready, MMC_ERR_STATE,
                "EwaldSelf needs an uploaded system and PrepareEwaldVariables");
    MMC_REQUIRE(self_energy, MMC_ERR_ARG, "NULL out pointer");
    double sq, sq2;
    if (!s.sums_valid)
        MMC_TRY(ctx_quiesce(ctx));
    MMC_TRY(s.charge_sums(&sq, &sq2));
    *self_energy = -s.bv.kappa * sq2 / sqrt(3.141592653589793) * s.bv.factor; // ewalds.jl:832
    return MMC_OK;
}

extern "C" int32_t mmc_potential_ewald(mmc_ctx *ctx, double lj_rcut, double qq_rcut,
                                       mmc_totals *tot)
{
    CTX_CHECK(ctx);
    MMC_REQUIRE(tot, MMC_ERR_ARG, "NULL out pointer");
    MMC_TRY(ctx_quiesce(ctx));
    MMC_TRY(ctx->sys.totals_ewald(lj_rcut, qq_rcut, tot));
    ctx->s_old = ctx->s_new = 0; // RecipLong inside wrote both arrays (energy.jl:1008)
    for (bool &v : ctx->m_valid) v = false;
    ctx->rc.valid = false;
    return MMC_OK;
}

extern "C" int32_t mmc_potential_wolf(mmc_ctx *ctx, double lj_rcut, double qq_rcut,
                                      mmc_totals *tot)
{
    CTX_CHECK(ctx);
    CTX_NO_VOLUME_TRIAL(ctx);
    DeviceSystem &s = ctx->sys;
    MMC_REQUIRE(tot, MMC_ERR_ARG, "NULL out pointer");
    MMC_REQUIRE(s.uploaded && s.ewald_ready, MMC_ERR_STATE,
                "potential needs an uploaded system and an EWALD (kappa, factor)");
    MMC_TRY(ctx_quiesce(ctx));
    std::vector<TotalsRaw> hts;
    MMC_TRY(s.pair_totals(lj_rcut, qq_rcut, hts));
    const TotalsRaw ht = hts[0];
    double sq, sq2;
    MMC_TRY(s.charge_sums(&sq, &sq2));
    const double factor = s.bv.factor, kappa = s.bv.kappa, r_cut = lj_rcut; // energy.jl:875
    mmc_totals t;
    memset(&t, 0, sizeof(t));
    t.energy = ht.lj_e / 2; // :895-897
    t.virial = ht.lj_v / 2;
    t.lj = ht.lj_e / 2;
    double totReal = ht.qq;
    totReal *= factor / 2; // :918
    t.energy += totReal; t.coulomb += totReal; // no virial term here (:919-920)
    t.real = totReal;
    // :924-930: sum_i sum_j q_i q_j erfc(kappa r_cut)/r_cut == (sum q)^2 erfc/r_cut, negated
    double prefactor = sq * sq * erfc(kappa * r_cut) / r_cut;
    prefactor *= -1;
    const double prefactor2 =
        (erfc(kappa * r_cut) / 2 / r_cut + kappa / sqrt(3.141592653589793)) * sq2; // :931-932
    t.energy += (prefactor - prefactor2) * factor;
    t.coulomb += (prefactor - prefactor2) * factor;
    t.self = (prefactor - prefactor2) * factor;
    t.n_overlap = ht.n_ovl;
    *tot = t;
    return MMC_OK;
}

// The five hot-path calls of one Loop() iteration in one evaluation (main.jl:491-593).
extern "C" int32_t mmc_trial_move(mmc_ctx *ctx, int64_t i, const double *com_new,
                                  const double *atoms_new, double lj_rcut, double qq_rcut,
                                  double d[4], int32_t *overlap)
{
    CTX_CHECK(ctx);
    CTX_NO_VOLUME_TRIAL(ctx);
    CTX_MOL(ctx, i);
    DeviceSystem &s = ctx->sys;
    MMC_REQUIRE(com_new && atoms_new && d && overlap, MMC_ERR_ARG, "NULL argument");
    MMC_REQUIRE(s.ewald_ready, MMC_ERR_STATE, "PrepareEwaldVariables has not run");
    MMC_REQUIRE(!ctx->trial_outstanding, MMC_ERR_STATE,
                "previous trial move not settled: call mmc_accept_move or mmc_reject_move");
    MMC_REQUIRE(s.h_cnt[i - 1] == 3, MMC_ERR_ASSERT, "AssertionError: n == 3 (ewalds.jl:740)");
    MMC_REQUIRE(s.k_sq_max == 27, MMC_ERR_ASSERT, "AssertionError: k_sq_max == 27 (ewalds.jl:742)");
    MMC_REQUIRE(s.nk == 5, MMC_ERR_ASSERT, "AssertionError: nk == 5 (ewalds.jl:743)");
    const int32_t m = (int32_t)(i - 1);
    ctx_mirror_catch_up(ctx);
    MoveRec *mv = ctx->h_move;
    mv->mol = (int32_t)i;
    mv->flags = 0;
    for (int k = 0; k < 3; k++)
        mv->com_new[k] = com_new[k];
    for (int k = 0; k < 9; k++)
        mv->atoms_new[k] = atoms_new[k];
    mmc_move_result res;
    ctx->rc.valid = false;
    // RecipMove starts from sumQExpNew, which Loop() keeps equal to sumQExpOld between moves
    // (main.jl:621,628): an unsettled RecipMove is dropped like a rejection
    ctx->s_new = ctx->s_old;
    if (ctx_server_applies(ctx, qq_rcut)) {
        auto &sv = ctx->srv;
        if (!sv.alive || sv.lj_rcut != lj_rcut || sv.qq_rcut != qq_rcut || sv.ovr != 0.5
            || sv.kappa != s.bv.kappa || sv.box != s.box
            || std::chrono::steady_clock::now() - sv.last_post > std::chrono::milliseconds(300))
            MMC_TRY(ctx_server_start(ctx, lj_rcut, qq_rcut, 0.5));
        unsigned long long *c = sv.h_cmd;
        double rec_new[12], rec_old[12];
        memcpy(rec_new, atoms_new, 72);
        memcpy(rec_new + 9, com_new, 24);
        memcpy(rec_old, &ctx->m_at[9 * (size_t)m], 72); // the mirror: the device holds it after
        memcpy(rec_old + 9, &ctx->m_com[3 * (size_t)m], 24); // the pending molecules of the command
        const int dst = ctx_free_sbuf(ctx);
        CMDW(c, CS_W_MOL) = (unsigned long long)(uint32_t)m;
        CMDW(c, CS_W_SBUF) = (unsigned long long)(uint32_t)(ctx->s_old | (dst << 8));
        ctx_fill_cmd_mol(ctx, m, rec_new, rec_old);
        MMC_TRY(ctx_cmd_pending(ctx));
        CtxEval ev;
        MMC_TRY(ctx_server_exec(ctx, CS_EVAL | CS_TWO | CS_RECIP, &ev));
        ctx->dirty.clear();
        ctx->m_valid[dst] = false;
        MMC_TRY(ctx_verify_smirror(ctx, dst, ev.s_sum));
        ctx->m_valid[dst] = true;
        ctx->s_new = dst;
        PartOut po;
        memset(&po, 0, sizeof(po));
        for (int st = 0; st < 2; st++) {
            po.lj_pot[st] = ev.lj_pot[st]; po.lj_vir[st] = ev.lj_vir[st];
            po.qq_pot[st] = ev.qq_pot[st]; po.ovl[st] = ev.ovl[st];
        }
        po.recip = ev.recip;
        mmc_combine_parts(&po, 1, s.bv.factor, &res);
    } else {
        MMC_TRY(ctx_normalize_sbufs(ctx));
        MMC_TRY(ctx_quiesce(ctx));
        const PairParams pp = mmc_pair_params(lj_rcut, qq_rcut, 0.0, 0.5, s.bv.kappa, false);
        dim3 grid((unsigned)ctx->n_parts, 1);
        k_move_eval<false><<<grid, MMC_BLOCK, 0, s.stream>>>(s.bv, ctx->d_move, nullptr, ctx->d_parts,
                                                      ctx->n_parts, pp, 0, s.rec, nullptr, 0u);
        MMC_HIP(hipGetLastError());
        MMC_TRY(s.sync());
        mmc_combine_parts(ctx->h_parts, ctx->n_parts, s.bv.factor, &res);
        ctx->s_new = 1;
        ctx->m_valid[1] = false;
    }
    d[0] = res.d_lj; d[1] = res.d_real; d[2] = res.d_recip; d[3] = res.d_vir;
    *overlap = res.overlap;
    ctx->trial_outstanding = true;
    ctx->trial_overlap = res.overlap;
    ctx->trial_mol = i;
    return MMC_OK;
}

extern "C" int32_t mmc_accept_move(mmc_ctx *ctx)
{
    CTX_CHECK(ctx);
    MMC_REQUIRE(ctx->trial_outstanding, MMC_ERR_STATE, "no trial move outstanding");
    MMC_REQUIRE(!ctx->trial_overlap, MMC_ERR_STATE,
                "an overlapped move is never accepted (main.jl:598)");
    // the molecule travels with the next evaluation; sumQExpOld <- sumQExpNew is a renaming
    (void)ctx_sync_mol(ctx, ctx->trial_mol, ctx->h_move->com_new, ctx->h_move->atoms_new);
    ctx->s_old = ctx->s_new; // main.jl:621
    ctx->trial_outstanding = false;
    return MMC_OK;
}

extern "C" int32_t mmc_reject_move(mmc_ctx *ctx)
{
    CTX_CHECK(ctx);
    MMC_REQUIRE(ctx->trial_outstanding, MMC_ERR_STATE, "no trial move outstanding");
    ctx->s_new = ctx->s_old; // main.jl:628
    ctx->trial_outstanding = false;
    return MMC_OK;
}

// Counters of the context's engine (tests and bench.py): out[0..7] = commands answered by the
// server, server launches, server retries, evaluations answered from the cache, RecipMoves answered
// from the speculative sum, speculative sums that were not used, evaluations by launch, whether the
// server is running, evaluations answered by the look-ahead, look-aheads posted.
extern "C" int32_t mmc_ctx_stats(mmc_ctx *ctx, int64_t out[10])
{
    MMC_REQUIRE(ctx && out, MMC_ERR_ARG, "NULL argument");
    out[0] = ctx->srv.n_cmds; out[1] = ctx->srv.n_launches; out[2] = ctx->srv.n_retries;
    out[3] = ctx->n_cache_hits; out[4] = ctx->n_spec_hits; out[5] = ctx->n_spec_miss;
    out[6] = ctx->n_launch_evals; out[7] = ctx->srv.alive ? 1 : 0;
    out[8] = ctx->n_la_hits; out[9] = ctx->n_la_posted;
    return MMC_OK;
}

// Test hook / measurement: the round trip of n empty commands through the running server (post,
// poll by every workgroup, one record per wave back): the floor under every served call.
extern "C" int32_t mmc_ctx_ping(mmc_ctx *ctx, int64_t n, double *us_avg)
{
    CTX_CHECK(ctx);
    MMC_REQUIRE(us_avg && n > 0, MMC_ERR_ARG, "bad argument");
    MMC_REQUIRE(ctx->srv.alive, MMC_ERR_STATE, "the context server is not running");
    CMDW(ctx->srv.h_cmd, CS_W_MOL) = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int64_t k = 0; k < n; k++) {
        CtxEval ev;
        MMC_TRY(ctx_server_exec(ctx, 0u, &ev));
    }
    *us_avg = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / (double)n;
    return MMC_OK;
}

// "server": -1 = use the persistent server when it applies (default), 0 = a launch per evaluation
extern "C" int32_t mmc_ctx_set_option(mmc_ctx *ctx, const char *key, int64_t value)
{
    CTX_CHECK(ctx);
    MMC_REQUIRE(key, MMC_ERR_ARG, "key is NULL");
    if (!strcmp(key, "server")) {
        MMC_TRY(ctx_server_stop(ctx));
        ctx->server_mode = value ? -1 : 0;
    } else {
        mmc_set_error("unknown option '%s'", key);
        return MMC_ERR_ARG;
    }
    return MMC_OK;
}

// ---- single-precision tolerance study (BASELINE configs[4]; not on the product path) -------------
#include "mmc_study.hpp"
#include <map>

// old3[3 a + d] = fp32 coordinate d of atom a of molecule i0
__global__ void k_study_gather_old(BatchView bv, const float *at, int i0, float *old3)
{
    const int t = threadIdx.x;
    if (t < 9)
        old3[t] = at[(t % 3) * bv.n_atoms + bv.first0[i0] + t / 3];
}

struct StudyBuffers {
    float *at = nullptr, *com = nullptr, *trial = nullptr; // [3 n_atoms], [3 n_mol], [12 + 9]
    float2 *Sf = nullptr;
    double *ek = nullptr;       // [nkvecs] + 1
    StudyMolOut *mol = nullptr; // [n_mol]
    int64_t n_atoms = 0, n_mol = 0;
};
static std::map<mmc_ctx *, StudyBuffers> g_study; // lives as long as its context

static StudyParams study_params(const DeviceSystem &s, double lj_rcut, double qq_rcut)
{
    StudyParams sp;
    sp.lj_gate_sq = (float)(lj_rcut * lj_rcut);
    sp.qq_gate_sq = (float)(qq_rcut * qq_rcut);
    sp.lj_slack_sq = (float)(lj_rcut * lj_rcut + 100);
    sp.qq_slack_sq = (float)(qq_rcut * qq_rcut + 100);
    sp.ovr = 0.5f;
    sp.kappa = (float)s.bv.kappa;
    sp.box = (float)s.box;
    return sp;
}

static int32_t study_prepare(mmc_ctx *ctx, StudyBuffers **out)
{
    DeviceSystem &s = ctx->sys;
    StudyBuffers &sb = g_study[ctx];
    if (sb.n_atoms != s.n_atoms || sb.n_mol != s.n_mol) {
        for (void *p : { (void *)sb.at, (void *)sb.com, (void *)sb.trial, (void *)sb.Sf,
                         (void *)sb.ek, (void *)sb.mol })
            if (p) (void)hipFree(p);
        sb = StudyBuffers();
        MMC_HIP(hipMalloc((void **)&sb.at, sizeof(float) * 3 * s.n_atoms));
        MMC_HIP(hipMalloc((void **)&sb.com, sizeof(float) * 3 * s.n_mol));
        MMC_HIP(hipMalloc((void **)&sb.trial, sizeof(float) * 24));
        MMC_HIP(hipMalloc((void **)&sb.Sf, sizeof(float2) * (s.nkvecs + 1)));
        MMC_HIP(hipMalloc((void **)&sb.ek, sizeof(double) * (s.nkvecs + 1)));
        MMC_HIP(hipMalloc((void **)&sb.mol, sizeof(StudyMolOut) * s.n_mol));
        sb.n_atoms = s.n_atoms;
        sb.n_mol = s.n_mol;
    }
    const int64_t n = s.n_atoms > s.n_mol ? s.n_atoms : s.n_mol;
    k_study_to_f32<<<(unsigned)((n + 255) / 256), 256, 0, s.stream>>>(s.bv, sb.at, sb.com);
    MMC_HIP(hipGetLastError());
    *out = &sb;
    return MMC_OK;
}

static void study_release(mmc_ctx *ctx)
{
    auto it = g_study.find(ctx);
    if (it == g_study.end())
        return;
    StudyBuffers &sb = it->second;
    for (void *p : { (void *)sb.at, (void *)sb.com, (void *)sb.trial, (void *)sb.Sf, (void *)sb.ek,
                     (void *)sb.mol })
        if (p) (void)hipFree(p);
    g_study.erase(it);
}

extern "C" int32_t mmc_study_f32_total(mmc_ctx *ctx, double lj_rcut, double qq_rcut,
                                       int32_t mixed, double out[6])
{
    CTX_CHECK(ctx);
    CTX_NO_VOLUME_TRIAL(ctx);
    DeviceSystem &s = ctx->sys;
    MMC_REQUIRE(out, MMC_ERR_ARG, "NULL out pointer");
    MMC_REQUIRE(s.uploaded && s.ewald_ready, MMC_ERR_STATE,
                "the study needs an uploaded system and an EWALD");
    MMC_REQUIRE(s.R == 1, MMC_ERR_UNSUPPORTED, "contexts only");
    StudyBuffers *sb;
    MMC_TRY(study_prepare(ctx, &sb));
    const StudyParams sp = study_params(s, lj_rcut, qq_rcut);
    if (mixed) {
        k_study_mol<double><<<(unsigned)s.n_mol, MMC_BLOCK, 0, s.stream>>>(s.bv, sb->at, sb->com, 0,
                                                                          nullptr, sp, sb->mol);
        k_study_recip_long<double><<<(unsigned)s.nkvecs, MMC_BLOCK, 0, s.stream>>>(
            s.bv, sb->at, sp.box, sb->Sf, sb->ek);
    } else {
        k_study_mol<float><<<(unsigned)s.n_mol, MMC_BLOCK, 0, s.stream>>>(s.bv, sb->at, sb->com, 0,
                                                                         nullptr, sp, sb->mol);
        k_study_recip_long<float><<<(unsigned)s.nkvecs, MMC_BLOCK, 0, s.stream>>>(
            s.bv, sb->at, sp.box, sb->Sf, sb->ek);
    }
    MMC_HIP(hipGetLastError());
    std::vector<StudyMolOut> hm(s.n_mol);
    std::vector<double> hk(s.nkvecs);
    MMC_HIP(hipMemcpyAsync(hm.data(), sb->mol, sizeof(StudyMolOut) * s.n_mol, hipMemcpyDeviceToHost,
                           s.stream));
    MMC_HIP(hipMemcpyAsync(hk.data(), sb->ek, sizeof(double) * s.nkvecs, hipMemcpyDeviceToHost,
                           s.stream));
    MMC_TRY(s.sync());
    // the sums over molecules / k-vectors in the accumulator precision of the study
    double lj = 0, vir = 0, qq = 0, rec = 0, n_ovl = 0;
    if (mixed) {
        for (auto &m : hm) { lj += m.lj_pot; vir += m.lj_vir; qq += m.qq_pot; n_ovl += m.ovl; }
        for (double e : hk) rec += e;
    } else {
        float flj = 0, fvir = 0, fqq = 0, frec = 0;
        for (auto &m : hm) {
            flj += (float)m.lj_pot; fvir += (float)m.lj_vir; fqq += (float)m.qq_pot; n_ovl += m.ovl;
        }
        for (double e : hk) frec += (float)e;
        lj = flj; vir = fvir; qq = fqq; rec = frec;
    }
    out[0] = 4 * lj / 2;              // energy.jl:289 and the halving of potential() (:985)
    out[1] = 24 * vir / 3.0 / 2;
    out[2] = qq * s.bv.factor / 2;    // energy.jl:1002-1003
    out[3] = rec * s.bv.factor;       // energy.jl:1009
    out[4] = n_ovl;
    out[5] = 0;
    return MMC_OK;
}

extern "C" int32_t mmc_study_f32_move(mmc_ctx *ctx, int64_t i, const double *com_new,
                                      const double *atoms_new, double lj_rcut, double qq_rcut,
                                      int32_t mixed, double d[3], int32_t *overlap)
{
    CTX_CHECK(ctx);
    CTX_NO_VOLUME_TRIAL(ctx);
    CTX_MOL(ctx, i);
    DeviceSystem &s = ctx->sys;
    MMC_REQUIRE(com_new && atoms_new && d && overlap, MMC_ERR_ARG, "NULL argument");
    MMC_REQUIRE(s.ewald_ready && s.R == 1, MMC_ERR_STATE, "the study needs an EWALD (contexts only)");
    auto it = g_study.find(ctx);
    MMC_REQUIRE(it != g_study.end() && it->second.n_atoms == s.n_atoms, MMC_ERR_STATE,
                "call mmc_study_f32_total first (it builds the fp32 structure factor)");
    StudyBuffers *sb = &it->second;
    float h[24];
    for (int k = 0; k < 9; k++) h[k] = (float)atoms_new[k];
    for (int k = 0; k < 3; k++) h[9 + k] = (float)com_new[k];
    const StudyParams sp = study_params(s, lj_rcut, qq_rcut);
    const int i0 = (int)i - 1;
    MMC_HIP(hipMemcpyAsync(sb->trial, h, sizeof(float) * 12, hipMemcpyHostToDevice, s.stream));
    // old state = the fp32 copy of the current coordinates (as of the last mmc_study_f32_total)
    float *old3 = sb->trial + 12;
    k_study_gather_old<<<1, 64, 0, s.stream>>>(s.bv, sb->at, i0, old3);
    if (mixed) {
        k_study_mol<double><<<1, MMC_BLOCK, 0, s.stream>>>(s.bv, sb->at, sb->com, i0, nullptr, sp,
                                                           sb->mol);
        k_study_mol<double><<<1, MMC_BLOCK, 0, s.stream>>>(s.bv, sb->at, sb->com, i0, sb->trial, sp,
                                                           sb->mol + 1);
        k_study_recip_move<double><<<1, MMC_BLOCK, 0, s.stream>>>(s.bv, sb->Sf, old3, sb->trial,
                                                                  i0, sp.box, sb->ek + s.nkvecs);
    } else {
        k_study_mol<float><<<1, MMC_BLOCK, 0, s.stream>>>(s.bv, sb->at, sb->com, i0, nullptr, sp,
                                                          sb->mol);
        k_study_mol<float><<<1, MMC_BLOCK, 0, s.stream>>>(s.bv, sb->at, sb->com, i0, sb->trial, sp,
                                                          sb->mol + 1);
        k_study_recip_move<float><<<1, MMC_BLOCK, 0, s.stream>>>(s.bv, sb->Sf, old3, sb->trial,
                                                                 i0, sp.box, sb->ek + s.nkvecs);
    }
    MMC_HIP(hipGetLastError());
    StudyMolOut hm[2];
    double hrec;
    MMC_HIP(hipMemcpyAsync(hm, sb->mol, sizeof(hm), hipMemcpyDeviceToHost, s.stream));
    MMC_HIP(hipMemcpyAsync(&hrec, sb->ek + s.nkvecs, sizeof(double), hipMemcpyDeviceToHost,
                           s.stream));
    MMC_TRY(s.sync());
    const int ov = hm[0].ovl || hm[1].ovl;
    if (mixed) {
        d[0] = 4 * (hm[1].lj_pot - hm[0].lj_pot);
        d[1] = ((hm[1].ovl ? 0.0 : hm[1].qq_pot) - (hm[0].ovl ? 0.0 : hm[0].qq_pot)) * s.bv.factor;
        d[2] = ov ? 0.0 : hrec * s.bv.factor;
    } else {
        d[0] = (double)(4.0f * ((float)hm[1].lj_pot - (float)hm[0].lj_pot));
        d[1] = (double)((((hm[1].ovl ? 0.0f : (float)hm[1].qq_pot)) -
                         (hm[0].ovl ? 0.0f : (float)hm[0].qq_pot)) * (float)s.bv.factor);
        d[2] = ov ? 0.0 : (double)((float)hrec * (float)s.bv.factor);
    }
    *overlap = ov;
    return MMC_OK;
}
