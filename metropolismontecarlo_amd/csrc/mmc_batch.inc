// mmc_batch.inc -- R independent replicas on one GPU: batched trial-move evaluation and the native
// host driver that does the sequential accept/reject of Loop() (Ewald/main.jl:487-644).
// Included by mmc_hip.hip.

#include <atomic>
#include <chrono>
#include <cmath>
#include <thread>
#include "mmc_state.hpp"
#include "mmc_solute_chain.hpp"

#define MMC_MAX_GROUPS 64
// option persistent = -1: replicas up to which the move server is used: up to one replica per
// compute unit, where it still wins (750 molecules, 256 replicas, 8 host threads: 11.6 us per step
// against 22.9 with launches; round 2, the replicas of a group stepped together: 18.1 against 29.6
// -- and the automatic choice stopped at 128).  It holds its compute units for the whole run.
#define MMC_SERVER_AUTO_MAX 256
#define MMC_GEN_MAX 16                 // steps whose proposals one k_propose launch generates
#define MMC_GEN_RING (MMC_GEN_MAX + 2) // + the previous step's record (pending commit) + slack
#define MMC_QUEUE_STRIDE 32            // a 128-byte line per group's ticket counter (mmc_batch::d_queue)

// Candidate lists of the move kernel's COM scan (mmc_cand.hpp): allocated when the batch first runs the
// wave kernel with one part per move; valid per replica while its displacement bound D_r says so.
#define MMC_CAND_EVERY 8 // launches of a range of replicas between two looks of k_cand_refresh
struct BatchCand {
    int enabled = 1;          // option "candidate_lists"
    int skin_milli = 2000;    // option "cand_skin": the lists' radius beyond the gate, in 1/1000 A
    bool tried = false;       // the allocation has been attempted (once per batch)
    int state = 4;            // mmc_batch_cand_stats: 0 off, 1 in use, 2 no memory, 3 not applicable, 4 not needed yet
    CandView v{};             // device arrays (idx NULL: none) and the budget they were built for
    void *block = nullptr;    // the one allocation behind them
    int64_t bytes = 0;
    uint32_t t_build = 0;     // threshold of the lists (com_quant_gate of gate + skin)
    uint32_t d_refresh = 0;   // a replica is rebuilt when D_r is above this
    uint64_t epoch = ~0ULL;   // DeviceSystem::comq_epoch the valid lists belong to
    bool dirty = true;        // something the lists depend on changed: every replica is stale
    int64_t refresh_launches = 0;
    struct Range { int64_t r0, nr; unsigned long long count; bool pending; };
    std::vector<Range> ranges; // the groups of replicas the driver launches, each with its own cadence
};

// The fixed solute of the batch (mmc_batch_set_solute, mmc_solute_chain.inc): n == 0 = none.
struct BatchSolute {
    int n = 0;                 // sites
    bool charged = false;      // some charge is not zero
    double mol[3 * (SOL_MAX_SITES + 1)] = { 0 }; // [n + 1][3]: sites, then the reference point c
    double charge[SOL_MAX_SITES] = { 0 }, eps[3 * SOL_MAX_SITES] = { 0 }, sig[3 * SOL_MAX_SITES] = { 0 };
    double q2 = 0.0;           // sum_a q_a^2 in site order (EwaldSelf)
    uint64_t hash = 0;         // mmc_state_info::solute_hash
    double *d_par = nullptr;   // [SOLC_PAR_DOUBLES] the device block of SoluteView, allocated on first use
    PartOut *h_parts = nullptr, *d_parts = nullptr; // [R] pinned + mapped: k_solute_move's record of every replica
    SoluteView view() const { return SoluteView{ d_par, n, charged ? 1 : 0 }; }
};

struct mmc_batch {
    DeviceSystem sys;
    BatchCand cand;
    BatchSolute sol;
    double lj_rcut = 0, qq_rcut = 0;
    int n_parts = 1;
    int kernel = 3;          // 3: choose per launch between 2 and 1 (default for homogeneous
                             // systems), 2: k_move_eval_wave, 1: k_move_eval_fast, 0: k_move_eval,
                             // 4: k_move_eval_lat (the move server's latency form, launch per step)
    int server_wgs = -1;     // workgroups per replica of the move server: -1 choose, 0 = one
                             // (k_move_server_wave), 2..4 = the latency server (k_move_server_lat)
    int wave_wgs = 0;        // workgroups of a k_move_eval_wave launch (0: 4 per CU = what its
                             // 128 VGPRs let be resident; more would queue behind the first)
    int n_cus = 256;
    bool fast_ok = false;    // the system qualifies for kernel 1
    bool rigid_only = true;  // every move committed so far was made on the device (k_propose):
                             // DeviceSystem::r_mol_max still bounds every molecule (a rigid move
                             // keeps the bound; mmc_batch_set_orientations raises it for its modes)
    int image_by_molecule = -1; // option: -1 where it is valid, 0 never (the per-pair minimum image)
    int zero_copy_moves = 0; // 1: kernels read the proposals from pinned host memory
    MoveRec *h_moves[2] = { nullptr, nullptr };  // pinned + mapped host staging
    MoveRec *hd_moves[2] = { nullptr, nullptr }; // device aliases of h_moves (zero-copy)
    MoveRec *d_moves[2] = { nullptr, nullptr };  // device-resident copies (default)
    PartOut *h_parts = nullptr, *d_parts = nullptr; // [R][MMC_MAX_PARTS], pinned + mapped
    int32_t *h_accept = nullptr, *d_accept = nullptr;
    int32_t *dev_accept = nullptr; // device copy of h_accept for the settle kernels (one DMA instead of a PCIe read per replica)
    int buf = 0;           // h_moves[buf] receives the next proposals
    bool has_prev = false; // h_moves[buf ^ 1] holds proposals that are not settled yet
    std::vector<uint8_t> s_cur;      // which S buffer is sumQExpOld, per replica
    std::vector<double> h_com, h_at; // host mirror of every replica (the driver proposes from it)
    bool mirror_valid = false;       // built on first use; stale after device-side proposals
    // device-side move generation (mmc_propose.hpp): per-replica flag byte and step sizes
    int device_moves = 0;
    MoveRec *d_ring = nullptr; // [ring_slots][R] device-generated move records, by step % ring_slots
    int ring_slots = MMC_GEN_RING; // (more where a launch takes more than MMC_GEN_MAX steps: batch_ensure_ring)
    double *d_quat = nullptr;  // [R][n_mol][4] orientations (only with mmc_batch_set_orientations)
    unsigned stamp = 0;        // last launch stamp handed out (PartOut::ovl[1])
    int64_t steps_done = 0;    // steps the native driver has run on this batch: the random streams
                               // continue from here (mmc_hip.h "Random streams")
    int eval_parts = 0;        // n_parts of the last mmc_batch_eval (mmc_batch_peek_part)
    // the reference's quaternion move generation (mmc_batch_set_orientations)
    int quat_mode = 0;         // 0 off, 1 faithful q_to_a, 2 Allen-Tildesley q_to_a
    double db[9] = { 0 };      // body-fixed sites
    // persistent move server (k_move_server_wave): small batches, device-side proposals
    int persistent = -1;       // -1: use it when it applies, 0: never, 1: insist (error if it cannot)
    unsigned long long *h_ctrl = nullptr, *hd_ctrl = nullptr; // pinned [R] control words
    unsigned long long *bar_ctrl = nullptr; // ... or device memory the host writes through the PCIe
                                            // BAR (mmc_bar_alloc): the server then polls local
                                            // memory instead of reading host memory over PCIe
    int32_t *h_timeout = nullptr, *hd_timeout = nullptr;      // pinned: a workgroup gave up waiting
    hipStream_t run_streams[MMC_MAX_GROUPS] = {}; // the native driver's streams and timing events,
    hipEvent_t run_events[MMC_MAX_GROUPS][2] = {}; // created on first use, kept until destroy
    void *pool = nullptr;              // the native driver's worker threads (WorkerPool, mmc_engine.inc), kept
    void (*pool_destroy)(void *) = nullptr; // between calls; joined by mmc_batch_destroy through this
    int steps_per_launch = 0;          // option "steps_per_launch": 0 = by size, 1, 2, 4, 8, 16
    int whole_call = 0;                // option "whole_call": 1 = where the kernel decides, a call of up
                                       // to MMC_STEPS_PER_LAUNCH_MAX steps in ONE launch per group (0: launches of steps_per_launch)
    int accept_on_device = -1;         // option "accept_on_device": -1 by host threads per launch, 0 host, 1 kernel          // option "accept_on_device": 0 keeps the decision on the host
    DecideConsts *d_decide = nullptr;  // what the kernel's own accept decision needs (Driver, device-side decisions)
    DecideConsts decide_host{};        // ... as last uploaded
    std::vector<double> temps;         // per-replica temperatures (mmc_batch_set_temperatures); empty = off
    double *d_temps = nullptr;         // ... on the device, [R] (DecideConsts::temps), allocated on first use
    unsigned *d_queue = nullptr;       // unit tickets of the kernel's multi-step launches: group g's at [MMC_QUEUE_STRIDE g]
    unsigned queue_base[MMC_MAX_GROUPS] = {}; // ... tickets taken so far (a launch takes one per unit)
    bool queue_reset = false;          // a run failed: tickets and counts may disagree
    int server_stall_ms = 0;   // test hook: the host delays the control words of step 2 by this much
    int64_t server_seq_offset = 0; // test hook: sequence numbers of the control words start here
    bool needs_reload = false; // a run failed half-way: coordinates, S buffers and the caller's
                               // energies may disagree until every replica has been set again
    std::vector<uint8_t> reloaded;
    int inject_torn = 0;       // test hook: corrupt the first N result copies before checking them
    bool vol_outstanding = false; // mmc_batch_volume_trial without its accept / reject yet
    bool vol_saved_fast_ok = false;
    int vol_saved_kernel = 0;
    std::vector<int32_t> pb_moved; // per-replica boxes: the replicas the outstanding volume trial moved
    int64_t trace_steps = 0;   // test hook: the driver records dU and the decision of the first N steps
    std::vector<double> trace_delta;   // [R][trace_steps] of the last run
    std::vector<uint8_t> trace_flags;  // bit 0 accepted, bit 1 overlap, bit 2 rotation
    uint8_t *h_flags = nullptr, *hd_flags = nullptr, *d_flags = nullptr;
    uint8_t *bar_flags = nullptr; // [R] device memory the host threads write through the BAR
                                  // (mmc_bar_alloc): no copy kernel between a step's launches
    double2 *h_steps = nullptr, *hd_steps = nullptr, *d_steps = nullptr;
    void *obs_buf = nullptr;    // device scratch of every observable call (obs_scratch, mmc_units.inc), grown on demand
    size_t obs_bytes = 0;
    void *obs_host = nullptr;   // ... and the pinned staging of a unit call's per-replica block (obs_staging)
    size_t obs_host_bytes = 0;
    int coulomb_style = MMC_COULOMB_EWALD; // mmc_batch_set_coulomb_style (main.jl:75)
    bool s_stale = false;       // the style went from Wolf back to Ewald: S(k) does not describe the
                                // coordinates until mmc_batch_recip_long / _potential_ewald rebuild it
    int local_stage = 1;        // the neighbour scans (local order, cavities, shell order, bond order, Voronoi cells and,
                                // always, network and rings: mmc_nbr.hpp) copy a replica's site positions to LDS
                                // where they fit (option "local_stage" = 0: never, the path of systems too large for it)
    int bond_chunk = 0;         // mmc_batch_bond_order: replicas per chunk of scratch records (0: by its budget)
    int ring_chunk = 0;         // mmc_batch_hbond_rings: replicas per launch with count_out or ring_out (0: by its budget)
    int voronoi_prune = 1;      // mmc_batch_voronoi: a face stops at the first plane that cannot reach it (0: walks them all; same bits)
    // save and resume (mmc_state.inc)
    uint64_t topology = 0;      // fingerprint of the topology the batch was created with (mmc_state_info::topology)
    int state_chunk = 0;        // mmc_batch_get_state / _set_state: replicas per chunk of staging (0: by its budget)
    int state_delivery = -1;    // ... 1: the kernels read and write the mapped pinned buffers themselves, 0: device
                                // staging and a copy, -1: what measured faster for each call (pack 1, unpack 0;
                                // profiles/checkpoint_bench.json -- the host's copy bounds both, so by a few per cent)
    void *st_h[2] = { nullptr, nullptr }, *st_hd[2] = { nullptr, nullptr }; // pinned + mapped staging, device aliases
    void *st_d[2] = { nullptr, nullptr };                                   // device staging
    size_t st_bytes = 0;        // of each of the four
    hipEvent_t st_ev[2] = {};   // buffer k's chunk has been packed and copied / unpacked
    uint8_t *d_state_cur = nullptr; // [R] device copy of s_cur for k_state_pack

    const MoveRec *dev_moves(int which) const
    {
        return zero_copy_moves ? hd_moves[which] : d_moves[which];
    }
};

static int32_t batch_pinned(void **h, void **d, size_t bytes)
{
    MMC_HIP(hipHostMalloc(h, bytes, hipHostMallocMapped | hipHostMallocCoherent));
    MMC_HIP(hipHostGetDevicePointer(d, *h, 0));
    memset(*h, 0, bytes);
    return MMC_OK;
}

static int batch_default_parts(int64_t R, int64_t n_mol)
{
    if (R >= 8192)
        return 1; // large batches: one unit per move (k_move_eval_wave)
    // enough workgroups to cover 256 CUs a few times over, but no thinner than ~190 molecules per
    // part (measured at 750 molecules, 32 chains: 5 parts 19.8 us per step, 9 parts 22.1, 3 parts
    // 22.5, 1 part 26.7; a single chain does not care)
    int64_t want = (2048 + R - 1) / R;
    int64_t cap = 1 + (n_mol + 187) / 188;
    int64_t p = want < cap ? want : cap;
    if (p > MMC_MAX_PARTS) p = MMC_MAX_PARTS;
    if (p < 1) p = 1;
    return (int)p;
}

extern "C" int32_t mmc_batch_create(int32_t device, void *hip_stream, int64_t n_replicas,
                                    int64_t n_mol, const double *com, const double *coords,
                                    const int64_t *atype, const double *charge, int64_t n_types,
                                    const double *eps, const double *sig, double box,
                                    double kappa, int64_t nk, int64_t k_sq_max, double factor,
                                    double lj_rcut, double qq_rcut, mmc_batch **out)
{
    MMC_REQUIRE(out, MMC_ERR_ARG, "out is NULL");
    *out = nullptr;
    MMC_REQUIRE(n_mol >= 1 && n_replicas >= 1, MMC_ERR_ARG, "n_mol and n_replicas must be >= 1");
    MMC_REQUIRE(n_mol < (1 << 27), MMC_ERR_ARG, "n_mol too large");
    MMC_REQUIRE(com && coords && atype && charge && eps && sig, MMC_ERR_ARG, "NULL array");
    MMC_REQUIRE(k_sq_max == 27, MMC_ERR_ASSERT, "AssertionError: k_sq_max == 27 (ewalds.jl:742)");
    MMC_REQUIRE(nk == 5, MMC_ERR_ASSERT, "AssertionError: nk == 5 (ewalds.jl:743)");
    MMC_REQUIRE(lj_rcut > 0 && qq_rcut > 0, MMC_ERR_ARG, "cutoffs must be > 0");
    // (Loop's `@assert totProps.LJ_rcut < box / 2`, main.jl:483, is the caller's: the NIST 20 A
    // configurations are evaluated at r_cut = box/2 exactly)
    MMC_REQUIRE(lj_rcut <= box / 2 && qq_rcut <= box / 2, MMC_ERR_ARG,
                "r_cut must not exceed box/2 (minimum image)");
    mmc_batch *b = new mmc_batch();
    std::vector<int64_t> fa(n_mol), la(n_mol);
    for (int64_t j = 0; j < n_mol; j++) { // RecipMove: n == 3 atoms per molecule (ewalds.jl:740)
        fa[j] = 3 * j + 1;
        la[j] = 3 * j + 3;
    }
    int32_t st = b->sys.init(device, hip_stream, n_replicas);
    b->sys.half_k = !getenv("MMC_FULL_K"); // (the switch is for A/B measurements: same results either way)
    if (st == MMC_OK)
        st = b->sys.upload(n_mol, 3 * n_mol, com, fa.data(), la.data(), coords, atype, charge,
                           n_types, eps, sig, box);
    if (st == MMC_OK)
        st = b->sys.prepare_ewald(kappa, nk, k_sq_max, box, factor, nullptr);
    const int64_t R = n_replicas;
    for (int k = 0; k < 2 && st == MMC_OK; k++) {
        st = batch_pinned((void **)&b->h_moves[k], (void **)&b->hd_moves[k], sizeof(MoveRec) * R);
        if (st == MMC_OK)
            st = b->sys.dmalloc((void **)&b->d_moves[k], sizeof(MoveRec) * R);
    }
    if (st == MMC_OK)
        st = batch_pinned((void **)&b->h_parts, (void **)&b->d_parts,
                          sizeof(PartOut) * R * MMC_MAX_PARTS);
    if (st == MMC_OK)
        st = batch_pinned((void **)&b->h_accept, (void **)&b->d_accept, sizeof(int32_t) * R);
    if (st == MMC_OK)
        st = b->sys.dmalloc((void **)&b->dev_accept, sizeof(int32_t) * R);
    if (st == MMC_OK)
        st = batch_pinned((void **)&b->h_flags, (void **)&b->hd_flags, (size_t)R);
    if (st == MMC_OK)
        st = batch_pinned((void **)&b->h_steps, (void **)&b->hd_steps, sizeof(double2) * R);
    if (st == MMC_OK)
        st = batch_pinned((void **)&b->h_ctrl, (void **)&b->hd_ctrl, sizeof(unsigned long long) * R);
    if (st == MMC_OK)
        b->bar_ctrl = (unsigned long long *)mmc_bar_alloc(sizeof(unsigned long long) * R); // (may be NULL)
    if (st == MMC_OK)
        b->bar_flags = (uint8_t *)mmc_bar_alloc((size_t)R); // (may be NULL)
    if (st == MMC_OK)
        st = batch_pinned((void **)&b->h_timeout, (void **)&b->hd_timeout, 64);
    if (st == MMC_OK)
        st = b->sys.dmalloc((void **)&b->d_flags, (size_t)R);
    if (st == MMC_OK)
        st = b->sys.dmalloc((void **)&b->d_steps, sizeof(double2) * R);
    if (st != MMC_OK) {
        mmc_batch_destroy(b);
        return st;
    }
    b->lj_rcut = lj_rcut;
    b->qq_rcut = qq_rcut;
    b->topology = state_topology(n_mol, atype, charge, n_types, eps, sig);
    b->n_parts = batch_default_parts(R, n_mol);
    // identical molecules and a cutoff the erfc table covers -> fast kernel, else the generic one
    b->fast_ok = b->sys.fast_table_ok(qq_rcut) && b->sys.n_mol <= MMC_WAVE_MAX_MOL;
    b->kernel = b->fast_ok ? 3 : 0;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
            b->n_cus = prop.multiProcessorCount;
    }
    b->s_cur.assign(R, 0);
    // (the host mirror h_com / h_at -- 72 KB per 750-molecule replica -- is built by
    // batch_refresh_mirror the first time a host-side proposal path needs it)
    *out = b;
    return MMC_OK;
}

extern "C" int32_t mmc_batch_destroy(mmc_batch *b)
{
    if (!b)
        return MMC_OK;
    if (b->pool && b->pool_destroy)
        b->pool_destroy(b->pool);
    b->pool = nullptr;
    (void)hipSetDevice(b->sys.device);
    if (b->sys.stream)
        (void)hipStreamSynchronize(b->sys.stream);
    for (int k = 0; k < 2; k++)
        if (b->h_moves[k])
            (void)hipHostFree(b->h_moves[k]);
    if (b->h_parts)
        (void)hipHostFree(b->h_parts);
    if (b->h_accept)
        (void)hipHostFree(b->h_accept);
    if (b->h_flags)
        (void)hipHostFree(b->h_flags);
    if (b->h_steps)
        (void)hipHostFree(b->h_steps);
    for (int g = 0; g < MMC_MAX_GROUPS; g++) {
        if (b->run_streams[g]) (void)hipStreamDestroy(b->run_streams[g]);
        for (int k = 0; k < 2; k++)
            if (b->run_events[g][k]) (void)hipEventDestroy(b->run_events[g][k]);
    }
    if (b->h_ctrl)
        (void)hipHostFree(b->h_ctrl);
    if (b->bar_ctrl)
        (void)hipFree(b->bar_ctrl);
    if (b->bar_flags)
        (void)hipFree(b->bar_flags);
    if (b->h_timeout)
        (void)hipHostFree(b->h_timeout);
    if (b->obs_buf)
        (void)hipFree(b->obs_buf);
    if (b->obs_host)
        (void)hipHostFree(b->obs_host);
    for (int k = 0; k < 2; k++) {
        if (b->st_h[k]) (void)hipHostFree(b->st_h[k]);
        if (b->st_d[k]) (void)hipFree(b->st_d[k]);
        if (b->st_ev[k]) (void)hipEventDestroy(b->st_ev[k]);
    }
    if (b->sol.h_parts) (void)hipHostFree(b->sol.h_parts);
    b->sys.release();
    delete b;
    return MMC_OK;
}

// (between mmc_batch_volume_trial and its accept / reject the batch holds the trial volume)
#define BATCH_NO_VOLUME_TRIAL(b)                                                                 \
    MMC_REQUIRE(!(b)->vol_outstanding, MMC_ERR_STATE,                                            \
                "volume move not settled: call mmc_batch_volume_accept or mmc_batch_volume_reject first")

// what a fixed solute fences (include/mmc_hip.h, "A fixed solute"): the energies would be another system's
#define BATCH_NO_SOLUTE(b, what)                                                                 \
    MMC_REQUIRE((b)->sol.n == 0, MMC_ERR_UNSUPPORTED,                                            \
                "%s: not available while a solute is set (mmc_batch_set_solute)", what)

#define BATCH_CHECK(b)                                                                           \
    MMC_REQUIRE((b) != nullptr, MMC_ERR_ARG, "batch is NULL");                                   \
    MMC_HIP(hipSetDevice((b)->sys.device))

// entry points that compute against the one shared box (include/mmc_hip.h, "Per-replica boxes")
#define BATCH_ONE_BOX(b, what)                                                                   \
    MMC_REQUIRE(!(b)->sys.pb.on, MMC_ERR_UNSUPPORTED,                                            \
                "%s: the batch has per-replica boxes (mmc_batch_set_boxes)", what)

// scope of the Wolf style (include/mmc_hip.h, "Coulomb style"): one box, NVT, no test particles
#define BATCH_NOT_WOLF(b, what)                                                                  \
    MMC_REQUIRE((b)->coulomb_style != MMC_COULOMB_WOLF, MMC_ERR_UNSUPPORTED,                     \
                "%s: not available in Wolf style (mmc_batch_set_coulomb_style)", what)
// paths that read S(k) (Ewald style only: Wolf style never looks at it)
#define BATCH_S_FRESH(b, what)                                                                   \
    MMC_REQUIRE(!((b)->s_stale && (b)->coulomb_style == MMC_COULOMB_EWALD), MMC_ERR_STATE,       \
                "%s: S(k) is stale after Wolf-style moves: call mmc_batch_recip_long (or "        \
                "mmc_batch_potential_ewald) first", what)

extern "C" int32_t mmc_batch_set_option(mmc_batch *b, const char *key, int64_t value)
{
    BATCH_CHECK(b);
    MMC_REQUIRE(key, MMC_ERR_ARG, "key is NULL");
    MMC_REQUIRE(!b->has_prev, MMC_ERR_STATE, "proposals outstanding: call mmc_batch_settle first");
    if (!strcmp(key, "parts")) {
        MMC_REQUIRE(value >= 1 && value <= MMC_MAX_PARTS, MMC_ERR_ARG, "parts outside 1..%d",
                    MMC_MAX_PARTS);
        b->n_parts = (int)value;
    } else if (!strcmp(key, "kernel")) {
        MMC_REQUIRE(!b->sys.pb.on || value == 1 || value == 3, MMC_ERR_UNSUPPORTED,
                    "per-replica boxes run kernel 1 only");
        MMC_REQUIRE(value >= 0 && value <= 4, MMC_ERR_ARG,
                    "kernel must be 0 (generic), 1 (workgroup per move), 2 (wave per move), "
                    "3 (1 or 2 by launch size) or 4 (latency form)");
        MMC_REQUIRE(value != 4 || b->coulomb_style != MMC_COULOMB_WOLF, MMC_ERR_UNSUPPORTED,
                    "kernel 4 (the latency form) has no Wolf instantiation");
        MMC_REQUIRE(value == 0 || b->fast_ok, MMC_ERR_UNSUPPORTED,
                    "the fast kernel needs identical molecules (same types and charges per "
                    "slot), at most %d of them, kappa <= %.2f and r_cut^2 + 100 <= %.0f",
                    MMC_WAVE_MAX_MOL, MMC_QQ_KAPPA_MAX, MMC_QQ_UMAX);
        b->kernel = (int)value;
    } else if (!strcmp(key, "wave_wgs")) {
        MMC_REQUIRE(value >= 0 && value <= (1 << 20), MMC_ERR_ARG, "wave_wgs outside 0..2^20");
        b->wave_wgs = (int)value;
    } else if (!strcmp(key, "server_wgs")) {
        MMC_REQUIRE(value >= -1 && value <= LAT_MAX_PARTS / LAT_WAVES && value != 1, MMC_ERR_ARG,
                    "server_wgs must be -1 (choose), 0 (one workgroup per replica) or 2..%d",
                    LAT_MAX_PARTS / LAT_WAVES);
        b->server_wgs = (int)value;
    } else if (!strcmp(key, "persistent")) {
        MMC_REQUIRE(value >= -1 && value <= 1, MMC_ERR_ARG, "persistent must be -1, 0 or 1");
        MMC_REQUIRE(!b->sys.pb.on || value != 1, MMC_ERR_UNSUPPORTED,
                    "per-replica boxes: the move server has one box");
        MMC_REQUIRE(value != 1 || b->coulomb_style != MMC_COULOMB_WOLF, MMC_ERR_UNSUPPORTED,
                    "the persistent move server has no Wolf instantiation (persistent = -1 uses launches)");
        b->persistent = (int)value;
    } else if (!strcmp(key, "server_seq_offset")) {
        MMC_REQUIRE(value >= 0, MMC_ERR_ARG, "server_seq_offset must be >= 0");
        b->server_seq_offset = value;
    } else if (!strcmp(key, "server_stall_ms")) {
        MMC_REQUIRE(value >= 0 && value <= 10000, MMC_ERR_ARG, "server_stall_ms outside 0..10000");
        b->server_stall_ms = (int)value;
    } else if (!strcmp(key, "inject_torn")) {
        b->inject_torn = (int)value;
    } else if (!strcmp(key, "local_stage")) {
        MMC_REQUIRE(value == 0 || value == 1, MMC_ERR_ARG, "local_stage must be 1 (where the positions fit) or 0 (never)");
        b->local_stage = (int)value;
    } else if (!strcmp(key, "bond_chunk")) {
        MMC_REQUIRE(value >= 0 && value <= (1 << 30), MMC_ERR_ARG, "bond_chunk must be 0 (by the scratch budget) or the replicas per chunk");
        b->bond_chunk = (int)value;
    } else if (!strcmp(key, "ring_chunk")) {
        MMC_REQUIRE(value >= 0 && value <= (1 << 30), MMC_ERR_ARG, "ring_chunk must be 0 (by the staging budget) or the replicas per launch");
        b->ring_chunk = (int)value;
    } else if (!strcmp(key, "state_chunk")) {
        MMC_REQUIRE(value >= 0 && value <= (1 << 30), MMC_ERR_ARG, "state_chunk must be 0 (by the staging budget) or the replicas per chunk");
        b->state_chunk = (int)value;
    } else if (!strcmp(key, "state_delivery")) {
        MMC_REQUIRE(value >= -1 && value <= 1, MMC_ERR_ARG, "state_delivery must be -1 (by call), 0 (device staging and a copy) or 1 (mapped pinned memory)");
        b->state_delivery = (int)value;
    } else if (!strcmp(key, "voronoi_prune")) {
        MMC_REQUIRE(value == 0 || value == 1, MMC_ERR_ARG, "voronoi_prune must be 1 (stop at the first plane out of reach) or 0 (never)");
        b->voronoi_prune = (int)value;
    } else if (!strcmp(key, "trace_steps")) {
        MMC_REQUIRE(value >= 0 && value * b->sys.R <= (1LL << 26), MMC_ERR_ARG, "trace_steps out of range");
        b->trace_steps = value;
    } else if (!strcmp(key, "zero_copy_moves")) {
        b->zero_copy_moves = value ? 1 : 0;
    } else if (!strcmp(key, "device_moves")) {
        MMC_REQUIRE(!b->sys.pb.on || value, MMC_ERR_UNSUPPORTED,
                    "per-replica boxes: the trial moves are drawn on the device");
        b->device_moves = value ? 1 : 0;
    } else if (!strcmp(key, "steps_per_launch")) {
        MMC_REQUIRE(value == 0 || value == 1 || value == 2 || value == 4 || value == 8 || value == 16, MMC_ERR_ARG,
                    "steps_per_launch must be 0 (by size), 1, 2, 4, 8 or 16");
        b->steps_per_launch = (int)value;
    } else if (!strcmp(key, "candidate_lists")) {
        MMC_REQUIRE(value == 0 || value == 1, MMC_ERR_ARG, "candidate_lists must be 0 (scan every centre of mass) or 1");
        b->cand.enabled = (int)value;
        b->cand.dirty = true;
    } else if (!strcmp(key, "cand_skin")) {
        MMC_REQUIRE(value >= 0 && value <= 100000, MMC_ERR_ARG, "cand_skin: 0..100000 (thousandths of an Angstrom)");
        b->cand.skin_milli = (int)value;
        b->cand.dirty = true;
    } else if (!strcmp(key, "whole_call")) {
        MMC_REQUIRE(value == 0 || value == 1, MMC_ERR_ARG, "whole_call must be 0 (launches of steps_per_launch) or 1 (one per call)");
        b->whole_call = (int)value;
    } else if (!strcmp(key, "accept_on_device")) {
        MMC_REQUIRE(value >= -1 && value <= 1, MMC_ERR_ARG, "accept_on_device must be -1 (by size), 0 (host) or 1 (kernel)");
        b->accept_on_device = (int)value;
    } else if (!strcmp(key, "image_by_molecule")) {
        MMC_REQUIRE(value == -1 || value == 0, MMC_ERR_ARG, "image_by_molecule must be -1 (where valid) or 0 (never)");
        b->image_by_molecule = (int)value;
    } else {
        mmc_set_error("unknown option '%s'", key);
        return MMC_ERR_ARG;
    }
    return MMC_OK;
}

extern "C" int32_t mmc_batch_set_parts(mmc_batch *b, int32_t n_parts)
{
    return mmc_batch_set_option(b, "parts", n_parts);
}

extern "C" int32_t mmc_batch_set_replica(mmc_batch *b, int64_t r, const double *com,
                                         const double *coords)
{
    BATCH_CHECK(b);
    MMC_REQUIRE(!b->has_prev, MMC_ERR_STATE, "proposals outstanding: call mmc_batch_settle first");
    BATCH_NO_VOLUME_TRIAL(b);
    MMC_REQUIRE(com && coords, MMC_ERR_ARG, "NULL array argument");
    MMC_TRY(b->sys.set_replica(r, com, coords));
    if (b->needs_reload) { // after a failed run: usable again once every replica has been set
        b->reloaded[r] = 1;
        bool all = true;
        for (uint8_t v : b->reloaded) all = all && v;
        if (all) {
            b->needs_reload = false;
            b->s_cur.assign(b->sys.R, 0); // (the caller runs RecipLong / potential next: both buffers)
        }
    }
    if (b->mirror_valid) {
        const int64_t n_mol = b->sys.n_mol;
        memcpy(&b->h_com[(size_t)r * n_mol * 3], com, sizeof(double) * n_mol * 3);
        memcpy(&b->h_at[(size_t)r * n_mol * 9], coords, sizeof(double) * n_mol * 9);
    }
    return MMC_OK;
}

extern "C" int32_t mmc_batch_get_replica(mmc_batch *b, int64_t r, double *com, double *coords,
                                         double *sum_old)
{
    BATCH_CHECK(b);
    MMC_REQUIRE(!b->has_prev, MMC_ERR_STATE, "proposals outstanding: call mmc_batch_settle first");
    MMC_TRY(b->sys.get_replica(r, com, coords));
    if (sum_old) {
        const BatchView &bv = b->sys.bv;
        std::vector<double> dev_order(2 * b->sys.nkvecs);
        MMC_HIP(hipMemcpy(dev_order.data(), bv.S + ((int64_t)r * 2 + b->s_cur[r]) * bv.nk_stride * 2,
                          sizeof(double) * 2 * b->sys.nkvecs, hipMemcpyDeviceToHost));
        b->sys.expand_S(dev_order.data(), sum_old); // the reference's NKVECS entries (ewalds.jl:90)
    }
    return MMC_OK;
}

static int32_t batch_solute_recip(mmc_batch *b, double *energies);  // mmc_solute_chain.inc
static int32_t batch_solute_totals(mmc_batch *b, mmc_totals *tot);

extern "C" int32_t mmc_batch_recip_long(mmc_batch *b, double *energies)
{
    BATCH_CHECK(b);
    MMC_REQUIRE(energies, MMC_ERR_ARG, "NULL out pointer");
    MMC_REQUIRE(!b->has_prev, MMC_ERR_STATE, "proposals outstanding: call mmc_batch_settle first");
    MMC_TRY(b->sys.recip_long_all(energies));
    if (b->sol.charged) // + S_sol(k): the energies and both buffers are those of the N + 1 system
        MMC_TRY(batch_solute_recip(b, energies));
    b->s_stale = false; // both buffers of every replica hold S(k) of its coordinates
    return MMC_OK;
}

extern "C" int32_t mmc_batch_potential_ewald(mmc_batch *b, mmc_totals *tot)
{
    BATCH_CHECK(b);
    MMC_REQUIRE(tot, MMC_ERR_ARG, "NULL out pointer");
    MMC_REQUIRE(!b->has_prev, MMC_ERR_STATE, "proposals outstanding: call mmc_batch_settle first");
    if (b->sol.n)
        MMC_TRY(batch_solute_totals(b, tot));
    else
        MMC_TRY(b->sys.totals_ewald(b->lj_rcut, b->qq_rcut, tot));
    b->s_stale = false; // RecipLong inside wrote both arrays (energy.jl:1008)
    return MMC_OK;
}

// ---- Coulomb style (main.jl:75 `Wolf`) -----------------------------------------------------------
extern "C" int32_t mmc_batch_set_coulomb_style(mmc_batch *b, int32_t style)
{
    BATCH_CHECK(b);
    MMC_REQUIRE(style == MMC_COULOMB_EWALD || style == MMC_COULOMB_WOLF, MMC_ERR_ARG,
                "style must be MMC_COULOMB_EWALD (0) or MMC_COULOMB_WOLF (1)");
    MMC_REQUIRE(!b->has_prev, MMC_ERR_STATE, "proposals outstanding: call mmc_batch_settle first");
    BATCH_NO_VOLUME_TRIAL(b);
    if (style == b->coulomb_style)
        return MMC_OK;
    if (style == MMC_COULOMB_WOLF) {
        BATCH_NO_SOLUTE(b, "Wolf style");
        MMC_REQUIRE(!b->sys.pb.on, MMC_ERR_UNSUPPORTED,
                    "Wolf style: the batch has per-replica boxes (mmc_batch_set_boxes)");
        MMC_REQUIRE(b->kernel != 4, MMC_ERR_UNSUPPORTED,
                    "Wolf style: kernel 4 (the latency form) has no Wolf instantiation");
        MMC_REQUIRE(b->persistent != 1, MMC_ERR_UNSUPPORTED,
                    "Wolf style: the persistent move server (option persistent = 1) has no Wolf "
                    "instantiation");
    } else {
        b->s_stale = true; // the Wolf moves left both S(k) buffers where they were
    }
    b->coulomb_style = style;
    return MMC_OK;
}

extern "C" int32_t mmc_batch_get_coulomb_style(mmc_batch *b, int32_t *style)
{
    MMC_REQUIRE(b && style, MMC_ERR_ARG, "NULL argument");
    *style = b->coulomb_style;
    return MMC_OK;
}

// potential() of the Wolf overload (energy.jl:864-943) for every replica: mmc_potential_wolf
// (mmc_ctx.inc) on the batch's pair-total kernels.  Neither style nor S(k) matter to it.
extern "C" int32_t mmc_batch_potential_wolf(mmc_batch *b, mmc_totals *tot)
{
    BATCH_CHECK(b);
    MMC_REQUIRE(tot, MMC_ERR_ARG, "NULL out pointer");
    MMC_REQUIRE(!b->has_prev, MMC_ERR_STATE, "proposals outstanding: call mmc_batch_settle first");
    BATCH_ONE_BOX(b, "mmc_batch_potential_wolf");
    BATCH_NO_SOLUTE(b, "mmc_batch_potential_wolf");
    DeviceSystem &s = b->sys;
    MMC_REQUIRE(s.uploaded && s.ewald_ready, MMC_ERR_STATE,
                "potential needs an uploaded system and an EWALD (kappa, factor)");
    std::vector<TotalsRaw> ht;
    MMC_TRY(s.pair_totals(b->lj_rcut, b->qq_rcut, ht));
    double sq, sq2;
    MMC_TRY(s.charge_sums(&sq, &sq2));
    const double factor = s.bv.factor, kappa = s.bv.kappa, r_cut = b->lj_rcut; // energy.jl:875
    // :924-930: sum_i sum_j q_i q_j erfc(kappa r_cut)/r_cut == (sum q)^2 erfc/r_cut, negated
    double prefactor = sq * sq * erfc(kappa * r_cut) / r_cut;
    prefactor *= -1;
    const double prefactor2 =
        (erfc(kappa * r_cut) / 2 / r_cut + kappa / sqrt(3.141592653589793)) * sq2; // :931-932
    for (int64_t r = 0; r < s.R; r++) {
        mmc_totals t;
        memset(&t, 0, sizeof(t));
        t.energy = ht[r].lj_e / 2; // :895-897
        t.virial = ht[r].lj_v / 2;
        t.lj = ht[r].lj_e / 2;
        double totReal = ht[r].qq;
        totReal *= factor / 2; // :918
        t.energy += totReal; t.coulomb += totReal; // no virial term here (:919-920)
        t.real = totReal;
        t.energy += (prefactor - prefactor2) * factor;
        t.coulomb += (prefactor - prefactor2) * factor;
        t.self = (prefactor - prefactor2) * factor;
        t.n_overlap = ht[r].n_ovl;
        tot[r] = t;
    }
    return MMC_OK;
}

// bring the host mirror back in step with the device after a run with device-side proposals
static int32_t batch_refresh_mirror(mmc_batch *b)
{
    if (b->mirror_valid)
        return MMC_OK;
    const int64_t n_mol = b->sys.n_mol;
    b->h_com.resize((size_t)b->sys.R * n_mol * 3);
    b->h_at.resize((size_t)b->sys.R * n_mol * 9);
    for (int64_t r = 0; r < b->sys.R; r++)
        MMC_TRY(b->sys.get_replica(r, &b->h_com[(size_t)r * n_mol * 3],
                                   &b->h_at[(size_t)r * n_mol * 9]));
    b->mirror_valid = true;
    return MMC_OK;
}

// mirror the commit of replica r's previous proposal on the host copy
static inline void batch_mirror_commit(mmc_batch *b, int64_t r, const MoveRec &m)
{
    const int64_t n_mol = b->sys.n_mol;
    memcpy(&b->h_com[((size_t)r * n_mol + (m.mol - 1)) * 3], m.com_new, sizeof(double) * 3);
    memcpy(&b->h_at[((size_t)r * n_mol + (m.mol - 1)) * 9], m.atoms_new, sizeof(double) * 9);
}

// the chosen molecule's current state, from the host mirror (== the device state once the pending
// commit of this replica has been applied to the mirror)
static inline void batch_fill_old(mmc_batch *b, int64_t r, MoveRec &m)
{
    const int64_t n_mol = b->sys.n_mol;
    memcpy(m.com_old, &b->h_com[((size_t)r * n_mol + (m.mol - 1)) * 3], sizeof(double) * 3);
    memcpy(m.atoms_old, &b->h_at[((size_t)r * n_mol + (m.mol - 1)) * 9], sizeof(double) * 9);
}

struct DevGen { // device-side proposals for this launch (mmc_propose.hpp)
    uint64_t seed;     // chain r draws from ChainKey{seed, replica0 + r} at counter rng_off + step
    uint64_t replica0;
    int64_t rng_off;
    int64_t step;      // the step this launch evaluates
    int n_gen;         // > 0: first generate the records of steps step .. step + n_gen - 1
    bool upload_steps; // h_steps of the range changed since the last launch
};

// The ring holds at least `slots` steps' records (between calls only: what it held is settled).
static int32_t batch_ensure_ring(mmc_batch *b, int slots = MMC_GEN_RING)
{
    if (b->d_ring && b->ring_slots >= slots)
        return MMC_OK;
    if (b->d_ring) { // a larger one: the records of a call never outlive it
        MMC_HIP(hipDeviceSynchronize());
        std::vector<void *> &a = b->sys.allocs;
        a.erase(std::remove(a.begin(), a.end(), (void *)b->d_ring), a.end());
        MMC_HIP(hipFree(b->d_ring));
        b->d_ring = nullptr;
    }
    slots = std::max(slots, (int)MMC_GEN_RING);
    MMC_TRY(b->sys.dmalloc((void **)&b->d_ring, sizeof(MoveRec) * (size_t)slots * b->sys.R));
    b->ring_slots = slots;
    return MMC_OK;
}

static inline const MoveRec *batch_ring_slot(const mmc_batch *b, int64_t step)
{
    return b->d_ring + (step % b->ring_slots) * b->sys.R;
}

// Which move kernel a launch of nr replicas x P parts runs (option "kernel"; 3 = by size).
// kernel 3: a wave per unit pays once a launch has a wave for every slot of the machine
// (4 per SIMD); below that the workgroup-per-move kernel, which spreads one move over 256
// lanes, has the shorter critical path (measured crossover: 2048 .. 8192 moves per launch)
static int batch_kernel_for(const mmc_batch *b, int64_t nr, int P)
{
    if (b->sys.pb.on) // per-replica boxes: the workgroup-per-move kernel is the one with a box per replica
        return 1;
    return b->kernel != 3 ? b->kernel : (nr * P >= (int64_t)16 * b->n_cus ? 2 : 1);
}

// A launch whose kernel makes the accept decision itself (DecideConsts, mmc_kernels.hpp).
struct DevDecide {
    const DecideConsts *dc; // device memory
    int64_t step;           // the chain step of this launch (with the call's offset): the Philox counter
    PartOut *parts;         // [R] where this launch's result records go (two slots alternate)
    bool fetch_flags;       // no BAR: bring the flag bytes the host wrote before the call's first launch
    int n_sub;              // steps of the chain this launch takes (> 1: one record for all of them)
    unsigned *queue;        // n_sub > 1: the group's unit tickets (k_move_eval_wave, wave_ticket), or null
    unsigned queue_base;    // ... tickets taken before this launch
};

// ---- candidate lists (mmc_cand.hpp) --------------------------------------------------------------
// Before the launches of a call that runs the wave kernel with one part per move, every stream of the
// batch idle: allocate on first use, fix the thresholds for the box and gates of the day, and mark every
// replica stale if anything the lists depend on has changed since they were valid.
static int32_t batch_cand_prepare(mmc_batch *b, const PairParams &pp)
{
    BatchCand &c = b->cand;
    DeviceSystem &s = b->sys;
    if (!c.enabled) {
        c.state = 0;
        return MMC_OK;
    }
    if (!s.bv.comq || s.pb.on || s.n_mol > MMC_WAVE_MAX_MOL) {
        c.state = 3;
        return MMC_OK;
    }
    if (!c.tried) {
        c.tried = true;
        const int64_t R = s.R, cqs = s.bv.cq_stride;
        auto up = [](int64_t x) { return (x + 255) / 256 * 256; };
        const int64_t b_stat = up(8 * MMC_CAND_STATS * R), b_d = up(4 * R), b_q0 = up(2 * 3 * cqs * R),
                      b_cnt = up(2 * cqs * R), b_idx = up(2 * (int64_t)MMC_CAND_CAP * s.n_mol * R);
        const int64_t total = b_stat + b_d + b_q0 + b_cnt + b_idx;
        size_t free_b = 0, total_b = 0;
        void *blk = nullptr;
        // (leave a sixteenth of the device, at least 1 GiB, to everything that allocates later)
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess
            && (size_t)total + std::max<size_t>(total_b / 16, (size_t)1 << 30) <= free_b
            && hipMalloc(&blk, (size_t)total) == hipSuccess) {
            s.allocs.push_back(blk);
            char *p = (char *)blk;
            c.v.stat = (unsigned long long *)p; p += b_stat;
            c.v.D = (uint32_t *)p; p += b_d;
            c.v.q0 = (uint16_t *)p; p += b_q0;
            c.v.cnt = (uint16_t *)p; p += b_cnt;
            c.v.idx = (uint16_t *)p;
            c.block = blk;
            c.bytes = total;
            // (the indices need no value: nothing reads a list before k_cand_refresh has written it,
            // and the move kernel clamps what it gathers by)
            MMC_HIP(hipMemsetAsync(blk, 0, (size_t)(total - b_idx), s.stream));
            c.dirty = true;
        } else {
            (void)hipGetLastError();
            c.state = 2;
        }
    }
    if (!c.v.idx)
        return MMC_OK;
    const double gate_sq = std::max(pp.lj_gate_sq, pp.qq_gate_sq), gate = std::sqrt(gate_sq);
    const double wide = gate + 1e-3 * c.skin_milli;
    const uint32_t t_build = com_quant_gate(wide * wide, s.box);
    const uint32_t budget = cand_budget(t_build, com_quant_gate(gate_sq, s.box));
    if (t_build != c.t_build || budget != c.v.budget) {
        c.t_build = t_build;
        c.v.budget = budget;
        c.dirty = true;
    }
    // Rebuilt when the bound has used three quarters of the budget: the molecules that have themselves
    // moved more than the last quarter scan in full until then, and a rebuild costs n_mol scans.
    c.d_refresh = (uint32_t)(((uint64_t)budget * 3 / 4) * ((uint64_t)budget * 3 / 4));
    c.state = budget > 0 ? 1 : 3;
    if (c.dirty || c.epoch != s.comq_epoch) {
        MMC_HIP(hipMemsetAsync(c.v.D, 0xff, sizeof(uint32_t) * (size_t)s.R, s.stream));
        MMC_HIP(hipStreamSynchronize(s.stream));
        c.dirty = false;
        c.epoch = s.comq_epoch;
        for (BatchCand::Range &g : c.ranges)
            g.pending = true;
    }
    return MMC_OK;
}

// A launch on `stream` that commits moves of replicas [r0, r0 + nr) WITHOUT keeping their bound (any
// kernel but the wave kernel with one part per move, or that kernel with the lists switched off): the
// replicas are stale from there on, in stream order.
static int32_t batch_cand_stale(mmc_batch *b, hipStream_t stream, int64_t r0, int64_t nr)
{
    if (b->cand.v.idx) {
        MMC_HIP(hipMemsetAsync(b->cand.v.D + r0, 0xff, sizeof(uint32_t) * (size_t)nr, stream));
        for (BatchCand::Range &g : b->cand.ranges) // (rebuilt at their next launch with lists, not at its turn)
            if (g.r0 < r0 + nr && r0 < g.r0 + g.nr)
                g.pending = true;
    }
    return MMC_OK;
}

// The view a launch of the wave kernel with one part per move takes for replicas [r0, r0 + nr), after
// enqueueing on the launch's own stream what keeps their lists fresh: k_cand_refresh at the range's
// first launch after anything went stale, then every MMC_CAND_EVERY launches (a replica with nothing
// to do costs one early exit).  Only speed depends on the cadence: a replica that is due scans in full.
static int32_t batch_cand_for_launch(mmc_batch *b, hipStream_t stream, int64_t r0, int64_t nr, CandView *out)
{
    BatchCand &c = b->cand;
    *out = CandView{};
    if (!c.enabled || !c.v.idx || c.v.budget == 0)
        return batch_cand_stale(b, stream, r0, nr);
    BatchCand::Range *g = nullptr;
    for (BatchCand::Range &x : c.ranges)
        if (x.r0 == r0 && x.nr == nr)
            g = &x;
    if (!g) {
        c.ranges.push_back(BatchCand::Range{ r0, nr, 0ULL, true });
        g = &c.ranges.back();
    }
    if (g->pending || g->count % MMC_CAND_EVERY == 0) {
        k_cand_refresh<<<(unsigned)nr, 256, 0, stream>>>(b->sys.bv, c.v, (int)r0, c.t_build, c.d_refresh);
        MMC_HIP(hipGetLastError());
        c.refresh_launches++;
        g->pending = false;
    }
    g->count++;
    *out = c.v;
    return MMC_OK;
}

// The form of a k_move_eval_wave launch: its five template arguments.  subst = several parts per move,
// which the host adds up and decides on: never with multi or ladder, which belong to the kernel's own
// decision.  20 of the 32 combinations exist.
struct WaveForm { bool subst, img, multi, wolf, ladder; };

// Enqueue one step for replicas [r0, r0 + nr): proposals h_moves[buf] -> device (or generated
// there when `dg` is given), then the fused move kernel.  `has_prev`: the previous proposals of
// these replicas are outstanding (moves[buf ^ 1], or the ring slot of step - 1).
// `before_kernel`: optional event recorded in front of the move kernel (kernel timing).
// `kernel`: batch_kernel_for of this launch's replicas and parts, from the caller.
static int32_t batch_launch(mmc_batch *b, hipStream_t stream, int64_t r0, int64_t nr, int P, int kernel,
                            int buf, bool has_prev, const PairParams &pp,
                            hipEvent_t before_kernel = nullptr, const DevGen *dg = nullptr,
                            unsigned stamp = 0, const DevDecide *dd = nullptr)
{
    DeviceSystem &s = b->sys;
    const MoveRec *cur, *prev;
    const uint8_t *flagv = nullptr;
    if (dg) {
        flagv = b->hd_flags;
        const double2 *stp = b->hd_steps;
        if (!b->zero_copy_moves) { // the flag bytes (and new step sizes) are all that crosses PCIe
            // The host threads have written the flag bytes into device memory themselves where the
            // device has a large BAR (Driver::proposals: posted writes, in order before this
            // launch's doorbell).  Otherwise a copy kernel reading the pinned host bytes -- not a
            // DMA packet: between two kernels of one stream a hipMemcpyAsync costs ~10 us of
            // stream time, a kernel ~2 + its 4.7 us.
            // (the kernel's own decisions, DevDecide: it keeps the flag bytes itself, in plain device
            // memory -- a byte stored into the BAR-mapped array cost the launch 9 of 260 us -- and
            // takes the host's only before the call's first launch)
            if (dd ? dd->fetch_flags : !b->bar_flags)
                k_fetch_bytes<<<(unsigned)((nr + 1023) / 1024), 256, 0, stream>>>(
                    b->d_flags + r0, b->hd_flags + r0, (int)nr);
            if (dg->upload_steps)
                MMC_HIP(hipMemcpyAsync(b->d_steps + r0, b->h_steps + r0, sizeof(double2) * nr,
                                       hipMemcpyHostToDevice, stream));
            flagv = b->bar_flags && !dd ? b->bar_flags : b->d_flags;
            stp = b->d_steps;
        }
        if (dg->n_gen > 0) {
            GenArgs ga;
            ga.steps = stp; ga.seed = dg->seed; ga.replica0 = dg->replica0;
            ga.rng_off = dg->rng_off; ga.step0 = dg->step; ga.n_gen = dg->n_gen;
            ga.ring = b->ring_slots; ga.ring_stride = s.R; ga.flag0 = flagv;
            ga.quat_mode = b->quat_mode;
            memcpy(ga.db, b->db, sizeof(ga.db));
            const int64_t n = nr * dg->n_gen;
            if (s.pb.on)
                k_propose<<<(unsigned)((n + 63) / 64), 64, 0, stream>>>(s.bv, s.rec, b->d_ring, ga, (int)r0,
                                                                        (int)nr, has_prev ? 1 : 0, s.pb_view());
            else
                k_propose<<<(unsigned)((n + 63) / 64), 64, 0, stream>>>(s.bv, s.rec, b->d_ring, ga,
                                                                        (int)r0, (int)nr, has_prev ? 1 : 0);
        }
        cur = batch_ring_slot(b, dg->step);
        prev = has_prev ? batch_ring_slot(b, dg->step + b->ring_slots - 1) : nullptr;
    } else {
        b->rigid_only = false; // the caller's proposals: nothing is known about their shape
        s.r_mol_max = INFINITY;
        if (!b->zero_copy_moves)
            MMC_HIP(hipMemcpyAsync(b->d_moves[buf] + r0, b->h_moves[buf] + r0,
                                   sizeof(MoveRec) * nr, hipMemcpyHostToDevice, stream));
        cur = b->dev_moves(buf);
        prev = has_prev ? b->dev_moves(buf ^ 1) : nullptr;
    }
    if (before_kernel)
        MMC_HIP(hipEventRecord(before_kernel, stream));
    // A fixed solute: its record of every replica of the launch, IN FRONT of the move kernel on its stream.
    // It needs the step's move records only, and it is over in microseconds: its records are in host
    // memory when the move kernel's first ones arrive, so the host still works through a launch's
    // records while the launch runs.  (Behind the move kernel the host could not complete one replica
    // before the whole launch had ended, and its pass over the records ran after the launch instead of
    // beside it; DESIGN.md, "A fixed solute".)
    if (b->sol.n)
        k_solute_move<<<(unsigned)((nr + SOLC_BLOCK / 16 - 1) / (SOLC_BLOCK / 16)), SOLC_BLOCK, 0, stream>>>(
            b->sol.view(), cur, s.qq_tab, s.fc, pp, s.box, b->sol.d_parts, (int)r0, (int)nr, stamp);
    dim3 grid((unsigned)P, (unsigned)nr);
    MMC_REQUIRE(!dd || (dg && P == 1 && !b->zero_copy_moves && kernel == 2), MMC_ERR_ASSERT,
                "the kernel's own accept decision needs device-side proposals, one part per move and the wave kernel");
    const bool wolf = b->coulomb_style == MMC_COULOMB_WOLF; // (never with kernel 4 or per-replica boxes)
    if (kernel != 2) // (their commits do not keep the candidate lists' bound)
        MMC_TRY(batch_cand_stale(b, stream, r0, nr));
    MMC_REQUIRE(!wolf || (kernel != 4 && !s.pb.on), MMC_ERR_ASSERT, "Wolf style reached a kernel without a Wolf form");
    using Yes = std::true_type;
    using No = std::false_type;
    if (kernel == 4) {
        // latency form: P workgroups of four parts each per replica, one record per workgroup
        MMC_REQUIRE(lat_applies(4 * P, (int)s.n_mol, (int)s.nkvecs), MMC_ERR_UNSUPPORTED,
                    "kernel 4 needs 4..%d parts (a multiple of 4) with at most %d molecules per pair "
                    "part", LAT_MAX_PARTS, LAT_MAXMOL);
        k_move_eval_lat<<<grid, LAT_WAVES * 64, 0, stream>>>(s.bv, s.rec, s.qq_tab, s.kpack, s.fc,
                                                             cur, prev, b->d_parts, 4 * P, pp, (int)r0,
                                                             flagv, stamp);
    } else if (kernel == 2) {
        // persistent workgroups: a few per CU, each wave loops over (replica, part) units
        const int64_t n_units = nr * P;
        int64_t wgs = (n_units + WV_MWAVES - 1) / WV_MWAVES;
        // (what the kernel's registers and LDS let be resident: WV_OCC waves on each of 4 SIMDs)
        const int64_t cap = b->wave_wgs > 0 ? b->wave_wgs
                                            : (int64_t)(4 * (wolf ? WV_OCC_WOLF : WV_OCC) / WV_MWAVES) * b->n_cus;
        if (wgs > cap) wgs = cap;
        // the minimum image of an atom pair from its molecule's: rigid device-made moves only,
        // and gate + 2 r_mol < box / 2 (mmc_wave_unit.inc, WV_IMG)
        // ... and (gate + 2 r_mol)^2 inside the slack of the pair tests, which that variant skips
        const bool img = dg && b->rigid_only && b->image_by_molecule != 0 &&
                         s.image_by_molecule(std::max(pp.lj_gate_sq, pp.qq_gate_sq)) &&
                         s.pairs_inside_slack(pp.qq_gate_sq, pp.qq_slack_sq) &&
                         s.pairs_inside_slack(pp.lj_gate_sq, pp.lj_slack_sq);
        // the forms that decide (dd: one part per move, above): several steps in one record, and under
        // per-replica temperatures the LADDER twins, which read DecideConsts::temps[r] (the driver has
        // put d_temps into *dd->dc)
        const WaveForm f{ P != 1, img, dd && dd->n_sub > 1, wolf, dd && !b->temps.empty() };
        CandView cvv{}; // candidate lists: the forms with one part per move keep and use them
        if (P == 1)
            MMC_TRY(batch_cand_for_launch(b, stream, r0, nr, &cvv));
        else
            MMC_TRY(batch_cand_stale(b, stream, r0, nr));
        auto launch = [&](auto subst, auto img_, auto multi, auto wolf_, auto ladder) {
            k_move_eval_wave<subst(), img_(), multi(), wolf_(), ladder()><<<(unsigned)wgs, WV_MWAVES * 64, 0, stream>>>(
                s.bv, s.rec, s.qq_tab, s.kpack, s.fc, cur, prev, dd ? dd->parts : b->d_parts, P, pp,
                (int)r0, (int)n_units, flagv, stamp, dd ? dd->dc : nullptr, dd ? (long long)dd->step : 0LL,
                dd ? dd->n_sub : 1, (int)(dg ? dg->step % b->ring_slots : 0), dd ? dd->queue : nullptr,
                dd ? dd->queue_base : 0u, cvv);
        };
        // (only what is named here exists: 4 x 4 forms with one part per move, 2 x 2 with several)
        auto pick = [&](auto subst, auto img_, auto multi) {
            if (f.ladder) {
                if constexpr (!subst()) {
                    if (f.wolf) launch(subst, img_, multi, Yes{}, Yes{});
                    else launch(subst, img_, multi, No{}, Yes{});
                }
            } else if (f.wolf) launch(subst, img_, multi, Yes{}, No{});
            else launch(subst, img_, multi, No{}, No{});
        };
        if (f.multi) {
            if (f.img) pick(No{}, Yes{}, Yes{}); else pick(No{}, No{}, Yes{});
        } else if (!f.subst) {
            if (f.img) pick(No{}, Yes{}, No{}); else pick(No{}, No{}, No{});
        } else {
            if (f.img) pick(Yes{}, Yes{}, No{}); else pick(Yes{}, No{}, No{});
        }
    } else if (kernel == 1) {
        auto launch = [&](auto wolf_, const double *qq_tab, auto... per_box) {
            k_move_eval_fast<wolf_()><<<grid, MMC_BLOCK, 0, stream>>>(s.bv, s.rec, qq_tab, s.kpack, s.fc, cur, prev,
                                                                     b->d_parts, P, pp, (int)r0, flagv, stamp,
                                                                     per_box...);
        };
        if (s.pb.on) launch(No{}, nullptr, s.pb_view());
        else if (wolf) launch(Yes{}, s.qq_tab);
        else launch(No{}, s.qq_tab);
    } else {
        auto launch = [&](auto wolf_) {
            k_move_eval<wolf_()><<<grid, MMC_BLOCK, 0, stream>>>(s.bv, cur, prev, b->d_parts, P, pp, (int)r0,
                                                                 s.rec, flagv, stamp);
        };
        if (wolf) launch(Yes{}); else launch(No{});
    }
    MMC_HIP(hipGetLastError());
    return MMC_OK;
}

// ---- persistent move server (k_move_server_wave) -----------------------------------------------
// Waves of a replica's workgroup: pair parts of at least 64 molecules (one scan block per wave),
// at most SRV_WAVES - 1 of them, plus the reciprocal part.  The workgroup is bound by VALU issue on
// its four SIMDs whatever the split (750 molecules, one chain: 2 waves 17.0 us per step, 3: 13.6,
// 4: 11.6, 5: 11.4, 6: 12.8, 8: 12.8), so a single chain takes 5; several chains take 8 (32
// chains: 14.6 us against 15.6-17.3 with 4-6).
static int batch_server_parts(int64_t n_mol, int64_t R)
{
    int64_t pairs = (n_mol + 63) / 64;
    const int64_t cap = R == 1 ? 4 : SRV_WAVES - 1;
    if (pairs > cap) pairs = cap;
    if (pairs < 1) pairs = 1;
    return (int)pairs + 1;
}

// Can this batch run its moves through the persistent server?  Device-side rigid proposals, the
// table kernel, and a compute unit per replica (a workgroup that is not resident yet only starts
// late -- replicas never wait for each other -- but there is nothing to gain beyond that).
static bool batch_server_applies(const mmc_batch *b)
{
    return b->fast_ok && b->kernel != 0 && b->device_moves && !b->quat_mode
           && b->sys.R <= (int64_t)b->n_cus;
}

// Workgroups per replica of the latency server (0: use k_move_server_wave).  Several workgroups of
// a replica each poll its control word: taken only while that stays a few dozen pollers, and while
// every workgroup can be resident on a compute unit of its own.
static int batch_lat_shape(const mmc_batch *b)
{
    const DeviceSystem &s = b->sys;
    int G = b->server_wgs;
    if (G < 0)
        G = s.R * 4 <= (int64_t)b->n_cus ? 4 : 2; // four while every workgroup has a compute unit to itself
                                                  // (measured, every replica at its own pace, 750 molecules, us
                                                  // per step with 2 / 4 workgroups: 16 chains 7.5 / 6.5, 32
                                                  // chains 7.6 / 6.6, 64 chains 8.0 / 7.0; 128 chains 9.6 with 2)
    while (G >= 2 && !lat_applies(4 * G, (int)s.n_mol, (int)s.nkvecs))
        G--;
    if (G < 2 && b->server_wgs < 0) {
        // a system too large for four workgroups (more than ~1660 molecules): as many as it takes
        // for every pair wave's range to fit its resident storage -- 21 for 10 000 molecules
        // (BASELINE configs[3]); the step is then as long as a small system's, where one workgroup
        // scanning everything takes three times as long
        G = (int)(((s.n_mol + LAT_MAXMOL - 1) / LAT_MAXMOL + 3 + LAT_WAVES - 1) / LAT_WAVES);
        while (G <= LAT_MAX_PARTS / LAT_WAVES && !lat_applies(4 * G, (int)s.n_mol, (int)s.nkvecs))
            G++;
        if (G > LAT_MAX_PARTS / LAT_WAVES)
            G = 0;
    }
    if (G < 2 || s.R * G > (int64_t)b->n_cus)
        return 0;
    return G;
}

static void batch_ctrl_clear(mmc_batch *b)
{
    memset(b->h_ctrl, 0, sizeof(unsigned long long) * b->sys.R);
    if (b->bar_ctrl) { // (the host only ever WRITES this memory: a read through the BAR takes microseconds)
        for (int64_t r = 0; r < b->sys.R; r++)
            ((volatile unsigned long long *)b->bar_ctrl)[r] = 0ULL;
        mmc_bar_flush();
    }
}

static int32_t batch_server_start(mmc_batch *b, hipStream_t stream, int waves, const PairParams &pp,
                                  uint64_t seed, uint64_t replica0, int64_t rng_off, int lat_wgs = 0)
{
    DeviceSystem &s = b->sys;
    MMC_TRY(batch_cand_stale(b, stream, 0, s.R)); // (the servers commit without the candidate lists' bound)
    if (lat_wgs > 0) {
        batch_ctrl_clear(b);
        memset(b->h_timeout, 0, 64);
        std::atomic_thread_fence(std::memory_order_seq_cst);
        ServerArgs sa;
        sa.ctrl = b->bar_ctrl ? b->bar_ctrl : b->hd_ctrl; sa.steps = b->hd_steps;
        sa.seed = seed; sa.replica0 = replica0; sa.rng_off = rng_off;
        sa.timeout_flag = b->hd_timeout;
        sa.seq_off = (uint64_t)b->server_seq_offset;
        k_move_server_lat<<<(unsigned)(s.R * lat_wgs), LAT_WAVES * 64, 0, stream>>>(
            s.bv, s.rec, s.qq_tab, s.kpack, s.fc, b->d_parts, LAT_WAVES * lat_wgs, pp, sa);
        MMC_HIP(hipGetLastError());
        return MMC_OK;
    }
    MMC_REQUIRE(waves >= 2 && waves <= SRV_WAVES, MMC_ERR_ARG, "server workgroups have 2..%d waves",
                SRV_WAVES);
    batch_ctrl_clear(b);
    memset(b->h_timeout, 0, 64);
    std::atomic_thread_fence(std::memory_order_seq_cst);
    ServerArgs sa;
    sa.ctrl = b->bar_ctrl ? b->bar_ctrl : b->hd_ctrl; sa.steps = b->hd_steps;
    sa.seed = seed; sa.replica0 = replica0; sa.rng_off = rng_off;
    sa.timeout_flag = b->hd_timeout;
    sa.seq_off = (uint64_t)b->server_seq_offset;
    k_move_server_wave<<<(unsigned)s.R, waves * 64, 0, stream>>>(
        s.bv, s.rec, s.qq_tab, s.kpack, s.fc, b->d_parts, waves, pp, sa);
    MMC_HIP(hipGetLastError());
    return MMC_OK;
}

// one control word: the step's sequence number (1-based), the stamp its results must carry, flags
static inline void batch_server_post(mmc_batch *b, int64_t r, int64_t seq, unsigned stamp, unsigned flags)
{
    const unsigned long long w = ((unsigned long long)(seq + b->server_seq_offset) << 40) // (mod 2^24)
                                 | ((unsigned long long)(stamp & MMC_STAMP_MASK) << 8) | (flags & 0xffu);
    if (b->bar_ctrl) {
        std::atomic_thread_fence(std::memory_order_release);
        ((volatile unsigned long long *)b->bar_ctrl)[r] = w;
        mmc_bar_flush();
    } else {
        __atomic_store_n(&b->h_ctrl[r], w, __ATOMIC_RELEASE);
    }
}

// Commit the outstanding proposals (h_moves[buf_prev]) of replicas [r0, r0+nr) whose h_accept
// flag is set, without evaluating new ones.
static int32_t batch_settle_range(mmc_batch *b, hipStream_t stream, int64_t r0, int64_t nr,
                                  const MoveRec *prev, bool sync = true)
{
    DeviceSystem &s = b->sys;
    // the accept words in device memory first: a block per replica reading its word from pinned host
    // memory is a PCIe read per replica (65536 replicas: 200 us of a run's fixed cost; one DMA: ~15)
    MMC_HIP(hipMemcpyAsync(b->dev_accept + r0, b->h_accept + r0, sizeof(int32_t) * nr, hipMemcpyHostToDevice, stream));
    k_settle<<<(unsigned)((nr + 15) / 16), 256, 0, stream>>>(s.bv, prev, b->dev_accept, (int)r0, (int)nr);
    if (s.rec)
        k_settle_rec<<<(unsigned)((nr + 15) / 16), 256, 0, stream>>>(s.bv, s.rec, prev, b->dev_accept, (int)r0, (int)nr,
                                                                     b->cand.enabled ? b->cand.v : CandView{});
    MMC_HIP(hipGetLastError());
    if (sync)
        MMC_HIP(hipStreamSynchronize(stream));
    return MMC_OK;
}

#define BATCH_USABLE(b)                                                                          \
    MMC_REQUIRE(!(b)->needs_reload, MMC_ERR_STATE,                                               \
                "a run on this batch failed half-way: set every replica again "                   \
                "(mmc_batch_set_replica) and recompute its energies before using it")

// include/mmc_hip.h, "Candidate lists"
extern "C" int32_t mmc_batch_cand_stats(mmc_batch *b, int64_t *out)
{
    BATCH_CHECK(b);
    MMC_REQUIRE(out, MMC_ERR_ARG, "NULL argument");
    const BatchCand &c = b->cand;
    for (int k = 0; k < 8; k++)
        out[k] = 0;
    if (c.v.idx) {
        std::vector<unsigned long long> h((size_t)b->sys.R * MMC_CAND_STATS);
        MMC_HIP(hipDeviceSynchronize());
        MMC_HIP(hipMemcpy(h.data(), c.v.stat, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
        for (int64_t r = 0; r < b->sys.R; r++)
            for (int k = 0; k < MMC_CAND_STATS; k++)
                out[k] += (int64_t)h[(size_t)r * MMC_CAND_STATS + k];
    }
    out[3] = c.bytes;
    out[4] = c.refresh_launches;
    out[5] = c.enabled ? c.state : 0;
    out[6] = c.v.budget;
    out[7] = c.t_build;
    return MMC_OK;
}

extern "C" int32_t mmc_cand_thresholds(double gate, double skin, double box, uint32_t *out)
{
    MMC_REQUIRE(out && gate > 0 && skin >= 0 && box > 0, MMC_ERR_ARG, "bad gate / skin / box");
    out[0] = com_quant_gate(gate * gate, box);
    out[1] = com_quant_gate((gate + skin) * (gate + skin), box);
    out[2] = cand_budget(out[1], out[0]);
    return MMC_OK;
}

extern "C" int32_t mmc_cand_within(int64_t n, const uint32_t *a2, const uint32_t *d2, uint32_t budget, uint8_t *out)
{
    MMC_REQUIRE(n >= 0 && a2 && d2 && out, MMC_ERR_ARG, "NULL argument");
    for (int64_t k = 0; k < n; k++)
        out[k] = cand_within(a2[k], d2[k], budget) ? 1 : 0;
    return MMC_OK;
}

extern "C" int32_t mmc_batch_eval(mmc_batch *b, const mmc_move *moves, mmc_move_result *results)
{
    BATCH_CHECK(b);
    BATCH_ONE_BOX(b, "mmc_batch_eval");
    BATCH_USABLE(b);
    BATCH_NO_VOLUME_TRIAL(b);
    BATCH_S_FRESH(b, "mmc_batch_eval");
    MMC_REQUIRE(moves && results, MMC_ERR_ARG, "NULL argument");
    MMC_REQUIRE(!(b->sol.n && b->kernel == 4), MMC_ERR_UNSUPPORTED,
                "a solute is set (mmc_batch_set_solute): kernel 4 does not evaluate it"); // (as the runs: run_plan)
    MMC_TRY(batch_refresh_mirror(b));
    DeviceSystem &s = b->sys;
    const int64_t R = s.R;
    MoveRec *cur = b->h_moves[b->buf];
    const MoveRec *prev = b->h_moves[b->buf ^ 1];
    for (int64_t r = 0; r < R; r++)
        MMC_REQUIRE(moves[r].mol >= 1 && moves[r].mol <= s.n_mol, MMC_ERR_ARG,
                    "replica %lld: molecule index %d outside 1..%lld", (long long)r,
                    moves[r].mol, (long long)s.n_mol);
    for (int64_t r = 0; r < R; r++) {
        const int acc = (b->has_prev && moves[r].accept_prev) ? 1 : 0;
        if (acc) {
            if (b->coulomb_style != MMC_COULOMB_WOLF)
                b->s_cur[r] ^= 1; // main.jl:621: the buffer RecipMove wrote becomes sumQExpOld
            batch_mirror_commit(b, r, prev[r]);
        }
        cur[r].mol = moves[r].mol;
        cur[r].flags = acc | (b->s_cur[r] << 1);
        memcpy(cur[r].com_new, moves[r].com_new, sizeof(double) * 3);
        memcpy(cur[r].atoms_new, moves[r].atoms_new, sizeof(double) * 9);
        batch_fill_old(b, r, cur[r]);
    }
    const PairParams pp = mmc_pair_params(b->lj_rcut, b->qq_rcut, 0.0, 0.5, s.bv.kappa, false);
    const unsigned stamp = ++b->stamp;
    // (kernel 4: "parts" counts waves, four to a workgroup, and a workgroup writes one record)
    const int P = b->kernel == 4 ? (b->n_parts + 3) / 4 : b->n_parts;
    const int kernel = batch_kernel_for(b, R, P);
    if (P == 1 && kernel == 2) // (the wave kernel, one part per move: candidate lists)
        MMC_TRY(batch_cand_prepare(b, pp));
    MMC_TRY(batch_launch(b, s.stream, 0, R, P, kernel, b->buf, b->has_prev, pp, nullptr, nullptr, stamp));
    MMC_TRY(s.sync());
    b->eval_parts = P;
    const int PS = P + (b->sol.n ? 1 : 0); // (a fixed solute: one more record, k_solute_move's)
    for (int64_t r = 0; r < R; r++) {
        PartOut parts[MMC_MAX_PARTS + 1];
        for (int q = 0; q < PS; q++)
            MMC_REQUIRE(part_copy_checked(q < P ? b->h_parts + r * P + q : b->sol.h_parts + r, stamp, &parts[q]),
                        MMC_ERR_HIP, "replica %lld part %d: result record incomplete after the "
                        "stream was synchronised (stamp/checksum mismatch)", (long long)r, q);
        mmc_combine_parts(parts, PS, s.bv.factor, &results[r]);
    }
    b->buf ^= 1;
    b->has_prev = true;
    return MMC_OK;
}

extern "C" int32_t mmc_batch_peek_part(mmc_batch *b, int64_t r, int32_t part, void *out64,
                                       uint32_t *stamp)
{
    BATCH_CHECK(b);
    MMC_REQUIRE(out64 && stamp, MMC_ERR_ARG, "NULL argument");
    MMC_REQUIRE(b->eval_parts > 0, MMC_ERR_STATE, "no mmc_batch_eval has run");
    MMC_REQUIRE(r >= 0 && r < b->sys.R && part >= 0 && part < b->eval_parts, MMC_ERR_ARG,
                "replica / part out of range");
    memcpy(out64, b->h_parts + r * b->eval_parts + part, sizeof(PartOut));
    *stamp = b->stamp & MMC_STAMP_MASK;
    return MMC_OK;
}

extern "C" int32_t mmc_batch_set_orientations(mmc_batch *b, const double *quat, const double *db,
                                              int32_t mode)
{
    BATCH_CHECK(b);
    BATCH_ONE_BOX(b, "mmc_batch_set_orientations");
    MMC_REQUIRE(!b->has_prev, MMC_ERR_STATE, "proposals outstanding: call mmc_batch_settle first");
    MMC_REQUIRE(mode >= 0 && mode <= 2, MMC_ERR_ARG, "mode must be 0 (off), 1 (faithful) or 2");
    DeviceSystem &s = b->sys;
    if (mode == 0) {
        b->quat_mode = 0;
        s.bv.quat = nullptr;
        return MMC_OK;
    }
    MMC_REQUIRE(quat && db, MMC_ERR_ARG, "NULL array argument");
    const int64_t n = s.n_mol;
    for (int64_t j = 0; j < n; j++) { // q_to_a's check (quaternions.jl:20-25: tol = 1e-6, exit())
        const double *q = quat + 4 * j;
        const double norm = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
        MMC_REQUIRE(std::fabs(norm - 1.0) <= 1.0e-6, MMC_ERR_ASSERT,
                    "quaternion normalization error %.17g (molecule %lld)", norm, (long long)(j + 1));
    }
    if (!b->d_quat)
        MMC_TRY(s.dmalloc((void **)&b->d_quat, sizeof(double) * 4 * n * s.R));
    MMC_HIP(hipMemcpyAsync(b->d_quat, quat, sizeof(double) * 4 * n, hipMemcpyHostToDevice, s.stream));
    if (s.R > 1) {
        dim3 g((unsigned)((4 * n + 255) / 256), (unsigned)(s.R - 1));
        k_broadcast<<<g, 256, 0, s.stream>>>(b->d_quat, 4 * n, (int)(4 * n));
        MMC_HIP(hipGetLastError());
    }
    MMC_TRY(s.sync());
    // DeviceSystem::r_mol_max must bound every site's distance from its COM in every state the
    // chains can reach, not only in the uploaded one (image_by_molecule trusts it).
    // mmc_space_fixed puts site a at COM + A^T db_a.  With n = |q|^2 <= 1 + 1e-6, the
    // Allen-Tildesley A is n times a rotation.  The faithful A differs from it in a[1][2] only, by
    // E = 2 q4 (q2 - q3), |E| <= sqrt(2) n, and a[1][2] multiplies db_a,y into z.  Hence
    // |A^T db_a| <= n |db_a| (mode 2) and n (|db_a| + sqrt(2) |db_a,y|) (mode 1).  The 1e-5
    // covers n and the norm's drift over a chain of unnormalised quaternion products.
    double reach = 0.0;
    for (int a = 0; a < 3; a++) {
        const double *v = db + 3 * a;
        const double len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        reach = std::max(reach, mode == 1 ? len + std::sqrt(2.0) * std::fabs(v[1]) : len);
    }
    s.r_mol_max = std::max(s.r_mol_max, reach * (1.0 + 1e-5));
    memcpy(b->db, db, sizeof(b->db));
    b->quat_mode = mode;
    s.bv.quat = b->d_quat;
    return MMC_OK;
}

extern "C" int32_t mmc_batch_get_orientations(mmc_batch *b, int64_t r, double *quat)
{
    BATCH_CHECK(b);
    MMC_REQUIRE(quat, MMC_ERR_ARG, "NULL out pointer");
    MMC_REQUIRE(!b->has_prev, MMC_ERR_STATE, "proposals outstanding: call mmc_batch_settle first");
    MMC_REQUIRE(b->quat_mode && b->d_quat, MMC_ERR_STATE, "no orientations set");
    MMC_REQUIRE(r >= 0 && r < b->sys.R, MMC_ERR_ARG, "replica out of range");
    const int64_t n = b->sys.n_mol;
    MMC_HIP(hipMemcpyAsync(quat, b->d_quat + r * 4 * n, sizeof(double) * 4 * n,
                           hipMemcpyDeviceToHost, b->sys.stream));
    return b->sys.sync();
}

#ifdef WV_STAMPS
// diagnostic build only: phase timestamps of the last k_move_eval_wave launch
extern "C" int32_t mmc_debug_stamps(uint64_t *out, int64_t n_units)
{
    MMC_HIP(hipDeviceSynchronize());
    MMC_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wv_stamps), sizeof(uint64_t) * WV_NSTAMP * n_units));
    return MMC_OK;
}
#endif

#ifdef LAT_PROFILE
// diagnostic build only: ticks per phase of the last k_move_server_lat run (replica 0's waves)
extern "C" int32_t mmc_debug_lat_profile(uint64_t *out /* [64][8] */)
{
    MMC_HIP(hipDeviceSynchronize());
    MMC_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lat_prof), sizeof(uint64_t) * 64 * 8));
    return MMC_OK;
}
#endif

extern "C" int32_t mmc_batch_settle(mmc_batch *b, const int32_t *accept)
{
    BATCH_CHECK(b);
    MMC_REQUIRE(accept, MMC_ERR_ARG, "NULL argument");
    BATCH_ONE_BOX(b, "mmc_batch_settle");
    if (!b->has_prev)
        return MMC_OK;
    DeviceSystem &s = b->sys;
    const MoveRec *prev = b->h_moves[b->buf ^ 1];
    for (int64_t r = 0; r < s.R; r++) {
        b->h_accept[r] = accept[r] ? 1 : 0;
        if (accept[r]) {
            if (b->coulomb_style != MMC_COULOMB_WOLF)
                b->s_cur[r] ^= 1;
            batch_mirror_commit(b, r, prev[r]);
        }
    }
    MMC_TRY(batch_settle_range(b, s.stream, 0, s.R, b->dev_moves(b->buf ^ 1)));
    b->has_prev = false;
    return MMC_OK;
}

extern "C" int32_t mmc_batch_volume_change(mmc_batch *b, double new_box, double new_kappa)
{
    BATCH_CHECK(b);
    BATCH_NO_SOLUTE(b, "mmc_batch_volume_change");
    BATCH_NOT_WOLF(b, "mmc_batch_volume_change");
    BATCH_ONE_BOX(b, "mmc_batch_volume_change");
    MMC_REQUIRE(!b->has_prev, MMC_ERR_STATE, "proposals outstanding: call mmc_batch_settle first");
    MMC_REQUIRE(!b->vol_outstanding, MMC_ERR_STATE,
                "volume move not settled: call mmc_batch_volume_accept or mmc_batch_volume_reject first");
    MMC_REQUIRE(b->lj_rcut <= new_box / 2 && b->qq_rcut <= new_box / 2, MMC_ERR_ARG,
                "r_cut must not exceed new_box/2 (minimum image)");
    DeviceSystem &s = b->sys;
    const double f = new_box / s.box; // same arithmetic as k_rescale -> the mirror stays bit-equal
    MMC_TRY(s.volume_change(new_box, new_kappa));
    const int64_t n_mol = s.n_mol;
    for (int64_t r = 0; b->mirror_valid && r < s.R; r++)
        for (int64_t j = 0; j < n_mol; j++) {
            double *c = &b->h_com[((size_t)r * n_mol + j) * 3];
            double *at = &b->h_at[((size_t)r * n_mol + j) * 9];
            for (int k = 0; k < 3; k++) {
                const double old = c[k], nw = old * f, d = nw - old;
                c[k] = nw;
                for (int a = 0; a < 3; a++)
                    at[3 * a + k] += d;
            }
        }
    b->fast_ok = s.fast_table_ok(b->qq_rcut) && s.n_mol <= MMC_WAVE_MAX_MOL;
    if (!b->fast_ok)
        b->kernel = 0;
    return MMC_OK;
}

// An NPT volume move of a one-replica batch without a host round trip (include/mmc_hip.h;
// volumeChange.jl:59-147): the DeviceSystem's snapshot (k_copy_segments, one launch each way)
// around mmc_batch_volume_change + potential().
extern "C" int32_t mmc_batch_volume_trial(mmc_batch *b, double new_box, double new_kappa, mmc_totals *tot)
{
    BATCH_CHECK(b);
    BATCH_NO_SOLUTE(b, "mmc_batch_volume_trial");
    BATCH_NOT_WOLF(b, "mmc_batch_volume_trial");
    BATCH_ONE_BOX(b, "mmc_batch_volume_trial");
    BATCH_USABLE(b);
    MMC_REQUIRE(tot, MMC_ERR_ARG, "NULL out pointer");
    MMC_REQUIRE(!b->has_prev, MMC_ERR_STATE, "proposals outstanding: call mmc_batch_settle first");
    BATCH_NO_VOLUME_TRIAL(b);
    MMC_REQUIRE(b->sys.R == 1, MMC_ERR_UNSUPPORTED,
                "a batch has one box: a volume move with its own decision needs a batch of ONE replica "
                "(independent NPT replicas are one batch each)");
    MMC_REQUIRE(new_box > 0 && new_kappa > 0, MMC_ERR_ARG, "box and kappa must be positive");
    MMC_REQUIRE(b->lj_rcut <= new_box / 2 && b->qq_rcut <= new_box / 2, MMC_ERR_ARG,
                "r_cut must not exceed new_box/2 (minimum image)");
    DeviceSystem &s = b->sys;
    MMC_TRY(s.snapshot_take());
    const bool fast_ok = b->fast_ok;
    const int kernel = b->kernel;
    // (the host mirror of the coordinates, where one exists, is not snapshotted: it is rebuilt from
    // the device when next needed)
    b->mirror_valid = false;
    int32_t st = mmc_batch_volume_change(b, new_box, new_kappa);
    if (st == MMC_OK)
        st = s.totals_ewald(b->lj_rcut, b->qq_rcut, tot);
    if (st != MMC_OK) { // leave the batch as it was
        (void)s.snapshot_restore();
        (void)s.sync();
        b->fast_ok = fast_ok;
        b->kernel = kernel;
        return st;
    }
    b->vol_saved_fast_ok = fast_ok;
    b->vol_saved_kernel = kernel;
    b->vol_outstanding = true;
    return MMC_OK;
}

extern "C" int32_t mmc_batch_volume_accept(mmc_batch *b)
{
    BATCH_CHECK(b);
    BATCH_NO_SOLUTE(b, "mmc_batch_volume_accept");
    BATCH_NOT_WOLF(b, "mmc_batch_volume_accept");
    BATCH_ONE_BOX(b, "mmc_batch_volume_accept");
    MMC_REQUIRE(b->vol_outstanding, MMC_ERR_STATE, "no volume move outstanding");
    b->vol_outstanding = false;
    b->sys.snap.valid = false;
    return MMC_OK;
}

extern "C" int32_t mmc_batch_volume_reject(mmc_batch *b)
{
    BATCH_CHECK(b);
    BATCH_NO_SOLUTE(b, "mmc_batch_volume_reject");
    BATCH_NOT_WOLF(b, "mmc_batch_volume_reject");
    BATCH_ONE_BOX(b, "mmc_batch_volume_reject");
    MMC_REQUIRE(b->vol_outstanding, MMC_ERR_STATE, "no volume move outstanding");
    MMC_TRY(b->sys.snapshot_restore());
    MMC_TRY(b->sys.sync()); // the next run uses the driver's own streams
    b->fast_ok = b->vol_saved_fast_ok;
    b->kernel = b->vol_saved_kernel;
    b->mirror_valid = false;
    b->vol_outstanding = false;
    return MMC_OK;
}

// qq_pair of table `tab` at kappa for n values of r^2 (mmc_batch_qq_table and _replica)
static int32_t eval_qq_table(mmc_batch *b, const double *tab, double kappa, const double *u, int64_t n,
                             double *out)
{
    MMC_REQUIRE(u && out && n >= 0, MMC_ERR_ARG, "bad argument");
    MMC_REQUIRE(tab, MMC_ERR_STATE, "no table built");
    if (n == 0)
        return MMC_OK;
    for (int64_t i = 0; i < n; i++)
        MMC_REQUIRE(u[i] > 0.0 && u[i] < MMC_QQ_UMAX, MMC_ERR_ARG,
                    "r^2 = %g outside the table's domain (0, %g)", u[i], MMC_QQ_UMAX);
    DeviceSystem &s = b->sys;
    // (plain hipMalloc/hipFree: a stream-ordered hipFreeAsync behind a D2H copy into pageable
    // memory let the next allocation reuse the buffer too early on ROCm 7.2)
    double *d_u;
    MMC_HIP(hipMalloc((void **)&d_u, sizeof(double) * 2 * n));
    hipError_t e = hipMemcpyAsync(d_u, u, sizeof(double) * n, hipMemcpyHostToDevice, s.stream);
    if (e == hipSuccess) {
        k_eval_qq_table<<<(unsigned)((n + 255) / 256), 256, 0, s.stream>>>(tab, kappa, d_u, d_u + n,
                                                                           (int)n);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(out, d_u + n, sizeof(double) * n, hipMemcpyDeviceToHost, s.stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(s.stream);
    (void)hipFree(d_u);
    MMC_REQUIRE(e == hipSuccess, MMC_ERR_HIP, "qq_table evaluation failed: %s",
                hipGetErrorString(e));
    return MMC_OK;
}

extern "C" int32_t mmc_batch_qq_table(mmc_batch *b, const double *u, int64_t n, double *out)
{
    BATCH_CHECK(b);
    BATCH_ONE_BOX(b, "mmc_batch_qq_table");
    return eval_qq_table(b, b->sys.qq_tab, b->sys.bv.kappa, u, n, out);
}

extern "C" int32_t mmc_batch_qq_table_replica(mmc_batch *b, int64_t replica, const double *u, int64_t n,
                                              double *out)
{
    BATCH_CHECK(b);
    const DeviceSystem &s = b->sys;
    MMC_REQUIRE(replica >= 0 && replica < s.R, MMC_ERR_ARG, "replica %lld out of range [0, %lld)",
                (long long)replica, (long long)s.R);
    if (!s.pb.on)
        return eval_qq_table(b, s.qq_tab, s.bv.kappa, u, n, out);
    return eval_qq_table(b, s.pb.tab + replica * MMC_QQ_TABLE_DOUBLES, s.pb.kappa[replica], u, n, out);
}

extern "C" int32_t mmc_batch_rdf(mmc_batch *b, int32_t site, int32_t numbins, uint64_t *hist)
{
    BATCH_CHECK(b);
    BATCH_ONE_BOX(b, "mmc_batch_rdf");
    MMC_REQUIRE(hist, MMC_ERR_ARG, "NULL out pointer");
    MMC_REQUIRE(!b->has_prev, MMC_ERR_STATE, "proposals outstanding: call mmc_batch_settle first");
    MMC_REQUIRE(numbins >= 1 && numbins <= 8192, MMC_ERR_ARG, "numbins outside 1..8192");
    MMC_REQUIRE(site < 3, MMC_ERR_ARG, "site must be < 0 (centre of mass) or an atom slot 0..2");
    DeviceSystem &s = b->sys;
    const size_t bytes = sizeof(unsigned long long) * (size_t)(numbins + 1);
    unsigned long long *d_hist;
    MMC_HIP(hipMalloc((void **)&d_hist, bytes));
    hipError_t e = hipMemsetAsync(d_hist, 0, bytes, s.stream);
    if (e == hipSuccess) {
        k_rdf<<<(unsigned)s.R, MMC_BLOCK, sizeof(unsigned int) * (numbins + 1), s.stream>>>(
            s.bv, site, numbins, d_hist);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(hist, d_hist, bytes, hipMemcpyDeviceToHost, s.stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(s.stream);
    (void)hipFree(d_hist);
    MMC_REQUIRE(e == hipSuccess, MMC_ERR_HIP, "rdf histogram failed: %s", hipGetErrorString(e));
    return MMC_OK;
}
