// mmc_state.inc -- save and resume (include/mmc_hip.h, "Save and resume"): the batch's state as one
// record per replica, packed and unpacked on the device (mmc_state.hpp) and moved in chunks through
// two pinned staging buffers, the kernel of one chunk running while the other chunk is copied.  The
// calls move records and check that the batch is configured for them; they configure nothing, and no
// code here decides, proposes or evaluates a move.  Included by mmc_hip.hip after mmc_tempering.inc.
#include "mmc_state.hpp"

#define MMC_STATE_BUDGET (256LL << 20) // staging of option "state_chunk" = 0: two pinned and two device buffers

extern "C" int32_t mmc_state_record_layout(const void *info_, int64_t *offsets, int64_t *record_bytes)
{
    const mmc_state_info *info = static_cast<const mmc_state_info *>(info_);
    MMC_REQUIRE(info && offsets && record_bytes, MMC_ERR_ARG, "NULL argument");
    MMC_REQUIRE(info->magic == MMC_STATE_MAGIC && info->version == MMC_STATE_VERSION, MMC_ERR_ARG,
                "not an mmc_state_info of version %d (magic %016llx, version %lld)", MMC_STATE_VERSION,
                (unsigned long long)info->magic, (long long)info->version);
    MMC_REQUIRE(info->n_mol >= 1 && info->n_mol < (1 << 27) && info->nkvecs >= 1 && info->nkvecs <= MMC_NK_STRIDE,
                MMC_ERR_ARG, "n_mol %lld or nkvecs %lld out of range", (long long)info->n_mol, (long long)info->nkvecs);
    const StateLayout L = state_layout(info->n_mol, info->nkvecs, info->quat_mode != 0);
    for (int k = 0; k < 8; k++)
        offsets[k] = L.off[k];
    *record_bytes = L.bytes;
    return MMC_OK;
}

static void state_fill_info(const mmc_batch *b, mmc_state_info *o)
{
    const DeviceSystem &s = b->sys;
    memset(o, 0, sizeof(*o));
    o->magic = MMC_STATE_MAGIC;
    o->version = MMC_STATE_VERSION;
    o->R = s.R; o->n_mol = s.n_mol; o->nkvecs = s.nkvecs; o->half_k = s.half_k ? 1 : 0;
    o->lj_rcut = b->lj_rcut; o->qq_rcut = b->qq_rcut;
    o->topology = b->topology;
    o->nk = s.nk; o->k_sq_max = s.k_sq_max; o->factor = s.bv.factor;
    o->coulomb_style = b->coulomb_style; o->s_stale = b->s_stale ? 1 : 0;
    o->per_box = s.pb.on ? 1 : 0; o->alpha = s.pb.on ? s.pb.alpha : 0.0;
    o->temps_on = b->temps.empty() ? 0 : 1;
    o->quat_mode = b->quat_mode;
    if (b->quat_mode)
        memcpy(o->db, b->db, sizeof(o->db));
    o->box = s.box; o->kappa = s.bv.kappa;
    o->steps_done = b->steps_done;
    o->r_mol_max = s.r_mol_max;
    o->rigid_only = b->rigid_only ? 1 : 0;
    o->solute_on = b->sol.n > 0 ? 1 : 0;
    o->solute_hash = b->sol.n > 0 ? b->sol.hash : 0;
}

extern "C" int32_t mmc_batch_state_info(mmc_batch *b, void *info)
{
    MMC_REQUIRE(b && info, MMC_ERR_ARG, "NULL argument");
    state_fill_info(b, static_cast<mmc_state_info *>(info));
    return MMC_OK;
}

// Replicas per chunk and the staging for them: two pinned (mapped) buffers and two device buffers,
// kept with the batch and grown on demand.
static int32_t state_stage(mmc_batch *b, int64_t nr, int64_t rec_bytes, int64_t *chunk_out)
{
    DeviceSystem &s = b->sys;
    int64_t chunk = b->state_chunk > 0 ? b->state_chunk : std::max<int64_t>(1, MMC_STATE_BUDGET / 4 / rec_bytes);
    chunk = std::min<int64_t>(std::min(chunk, nr), 65535); // (a launch's grid is (slabs, replicas of the chunk))
    const size_t need = (size_t)(chunk * rec_bytes);
    if (need > b->st_bytes) {
        MMC_TRY(s.sync());
        for (int k = 0; k < 2; k++) {
            if (b->st_h[k]) (void)hipHostFree(b->st_h[k]);
            if (b->st_d[k]) (void)hipFree(b->st_d[k]);
            b->st_h[k] = b->st_hd[k] = b->st_d[k] = nullptr;
        }
        b->st_bytes = 0;
        for (int k = 0; k < 2; k++) {
            MMC_HIP(hipHostMalloc(&b->st_h[k], need, hipHostMallocMapped | hipHostMallocCoherent));
            MMC_HIP(hipHostGetDevicePointer(&b->st_hd[k], b->st_h[k], 0));
            MMC_HIP(hipMalloc(&b->st_d[k], need));
        }
        b->st_bytes = need;
    }
    for (int k = 0; k < 2; k++)
        if (!b->st_ev[k])
            MMC_HIP(hipEventCreateWithFlags(&b->st_ev[k], hipEventDisableTiming));
    if (!b->d_state_cur)
        MMC_TRY(s.dmalloc((void **)&b->d_state_cur, (size_t)s.R));
    *chunk_out = chunk;
    return MMC_OK;
}

static StateArgs state_args(const mmc_batch *b, const StateLayout &L)
{
    const DeviceSystem &s = b->sys;
    StateArgs a{};
    a.off_com = L.off[3]; a.off_coords = L.off[4]; a.off_S = L.off[5]; a.off_quat = L.off[6]; a.off_end = L.off[7];
    a.rec_bytes = L.bytes;
    a.n_slabs = (int)((s.n_mol + ST_SLAB - 1) / ST_SLAB);
    a.quat = b->quat_mode != 0;
    a.per_box = s.pb.on ? 1 : 0;
    a.d_box = s.pb.on ? s.pb.d_box : nullptr;
    a.box = s.box;
    a.d_temps = b->temps.empty() ? nullptr : b->d_temps;
    a.cur = b->d_state_cur;
    a.flags = (s.pb.on ? ST_FLAG_PER_BOX : 0u) | (b->temps.empty() ? 0u : ST_FLAG_TEMPS) | (b->quat_mode ? ST_FLAG_QUAT : 0u);
    return a;
}

#define STATE_RANGE(b, r0, nr)                                                                   \
    MMC_REQUIRE((r0) >= 0 && (nr) >= 0 && (r0) <= (b)->sys.R && (nr) <= (b)->sys.R - (r0), MMC_ERR_ARG, \
                "replicas [%lld, %lld) outside 0..%lld", (long long)(r0), (long long)((r0) + (nr)), (long long)(b)->sys.R)

extern "C" int32_t mmc_batch_get_state(mmc_batch *b, int64_t r0, int64_t nr, void *records)
{
    BATCH_CHECK(b);
    BATCH_BETWEEN_MOVES(b);
    BATCH_USABLE(b);
    STATE_RANGE(b, r0, nr);
    MMC_REQUIRE(records || nr == 0, MMC_ERR_ARG, "NULL argument");
    if (nr == 0)
        return MMC_OK;
    DeviceSystem &s = b->sys;
    MMC_REQUIRE(s.uploaded && s.ewald_ready, MMC_ERR_STATE, "no prepared system");
    const StateLayout L = state_layout(s.n_mol, s.nkvecs, b->quat_mode != 0);
    int64_t chunk = 0;
    MMC_TRY(state_stage(b, nr, L.bytes, &chunk));
    MMC_TRY(tempering_upload(b)); // (allocates d_temps where the array was set but never uploaded)
    for (int64_t r = 0; r < s.R; r++)
        b->s_cur[r] &= 1;
    MMC_HIP(hipMemcpy(b->d_state_cur, b->s_cur.data(), (size_t)s.R, hipMemcpyHostToDevice));
    StateArgs a = state_args(b, L);
    const bool direct = b->state_delivery != 0; // (-1: the pack kernel writes the mapped pinned buffer itself)
    uint8_t *out = static_cast<uint8_t *>(records);
    const int64_t n_chunks = (nr + chunk - 1) / chunk;
    for (int64_t c = 0; c <= n_chunks; c++) {
        const int k = (int)(c & 1);
        if (c < n_chunks) { // pack chunk c into buffer k ...
            const int64_t n = std::min(chunk, nr - c * chunk);
            a.r0 = (int)(r0 + c * chunk);
            const dim3 grid((unsigned)a.n_slabs, (unsigned)n);
            uint8_t *dst = static_cast<uint8_t *>(direct ? b->st_hd[k] : b->st_d[k]);
            if (s.rec)
                k_state_pack<true><<<grid, ST_BLOCK, 0, s.stream>>>(s.bv, s.rec, a, dst);
            else
                k_state_pack<false><<<grid, ST_BLOCK, 0, s.stream>>>(s.bv, s.rec, a, dst);
            MMC_HIP(hipGetLastError());
            if (!direct)
                MMC_HIP(hipMemcpyAsync(b->st_h[k], b->st_d[k], (size_t)(n * L.bytes), hipMemcpyDeviceToHost, s.stream));
            MMC_HIP(hipEventRecord(b->st_ev[k], s.stream));
        }
        if (c > 0) { // ... while chunk c - 1 leaves buffer k ^ 1
            const int64_t n = std::min(chunk, nr - (c - 1) * chunk);
            MMC_HIP(hipEventSynchronize(b->st_ev[k ^ 1]));
            memcpy(out + (c - 1) * chunk * L.bytes, b->st_h[k ^ 1], (size_t)(n * L.bytes));
        }
    }
    return MMC_OK;
}

static int32_t state_check_info(const mmc_batch *b, const mmc_state_info *in)
{
    mmc_state_info me;
    state_fill_info(b, &me);
    MMC_REQUIRE(in->magic == MMC_STATE_MAGIC && in->version == MMC_STATE_VERSION, MMC_ERR_ARG,
                "not an mmc_state_info of version %d (magic %016llx, version %lld)", MMC_STATE_VERSION,
                (unsigned long long)in->magic, (long long)in->version);
#define ST_SAME_I(f) MMC_REQUIRE(in->f == me.f, MMC_ERR_ARG, "state of another system: " #f " is %lld, the batch has %lld", \
                                 (long long)in->f, (long long)me.f)
#define ST_SAME_D(f) MMC_REQUIRE(in->f == me.f, MMC_ERR_ARG, "state of another system: " #f " is %.17g, the batch has %.17g", \
                                 in->f, me.f)
    ST_SAME_I(n_mol); ST_SAME_I(nkvecs); ST_SAME_I(half_k); ST_SAME_D(lj_rcut); ST_SAME_D(qq_rcut);
    MMC_REQUIRE(in->topology == me.topology, MMC_ERR_ARG,
                "state of another system: topology fingerprint %016llx, the batch has %016llx",
                (unsigned long long)in->topology, (unsigned long long)me.topology);
    ST_SAME_I(nk); ST_SAME_I(k_sq_max); ST_SAME_D(factor);
#undef ST_SAME_I
#undef ST_SAME_D
#define ST_MODE(cond, ...) MMC_REQUIRE(cond, MMC_ERR_STATE, "the batch is not configured for this state: " __VA_ARGS__)
    ST_MODE(in->coulomb_style == me.coulomb_style, "Coulomb style %lld, the batch has %lld (mmc_batch_set_coulomb_style)",
            (long long)in->coulomb_style, (long long)me.coulomb_style);
    ST_MODE(in->s_stale == me.s_stale, "s_stale %lld, the batch has %lld", (long long)in->s_stale, (long long)me.s_stale);
    ST_MODE(in->per_box == me.per_box, "per-replica boxes %s, the batch has them %s (mmc_batch_set_boxes)",
            in->per_box ? "on" : "off", me.per_box ? "on" : "off");
    ST_MODE(!in->per_box || in->alpha == me.alpha, "alpha %.17g, the batch has %.17g", in->alpha, me.alpha);
    ST_MODE(in->temps_on == me.temps_on, "temperatures %s, the batch has them %s (mmc_batch_set_temperatures)",
            in->temps_on ? "on" : "off", me.temps_on ? "on" : "off");
    ST_MODE(in->quat_mode == me.quat_mode, "orientation mode %lld, the batch has %lld (mmc_batch_set_orientations)",
            (long long)in->quat_mode, (long long)me.quat_mode);
    ST_MODE(!in->quat_mode || !memcmp(in->db, me.db, sizeof(me.db)), "the body-fixed sites differ (mmc_batch_set_orientations)");
    ST_MODE(in->per_box || (in->box == me.box && in->kappa == me.kappa),
            "box %.17g and kappa %.17g, the batch has %.17g and %.17g (mmc_batch_volume_change)", in->box, in->kappa,
            me.box, me.kappa);
    ST_MODE(in->solute_on == me.solute_on && in->solute_hash == me.solute_hash,
            "solute %s (hash %016llx), the batch has %s (hash %016llx) (mmc_batch_set_solute)", in->solute_on ? "set" : "not set",
            (unsigned long long)in->solute_hash, me.solute_on ? "one" : "none", (unsigned long long)me.solute_hash);
#undef ST_MODE
    return MMC_OK;
}

extern "C" int32_t mmc_batch_set_state(mmc_batch *b, const void *info_, int64_t r0, int64_t nr, const void *records)
{
    BATCH_CHECK(b);
    const mmc_state_info *info = static_cast<const mmc_state_info *>(info_);
    MMC_REQUIRE(info, MMC_ERR_ARG, "NULL argument");
    MMC_TRY(state_check_info(b, info));
    BATCH_BETWEEN_MOVES(b);
    STATE_RANGE(b, r0, nr);
    MMC_REQUIRE(records || nr == 0, MMC_ERR_ARG, "NULL argument");
    DeviceSystem &s = b->sys;
    MMC_REQUIRE(s.uploaded && s.ewald_ready, MMC_ERR_STATE, "no prepared system");
    const int64_t R = s.R;
    const StateLayout L = state_layout(s.n_mol, s.nkvecs, b->quat_mode != 0);
    const uint8_t *in = static_cast<const uint8_t *>(records);
    auto field = [&](int64_t y, int k) { // (the caller's memory need not be aligned)
        double v;
        memcpy(&v, in + y * L.bytes + L.off[k], sizeof(v));
        return v;
    };
    for (int64_t y = 0; y < nr; y++) { // what the batch's own setters refuse, before anything is changed
        if (s.pb.on)
            MMC_REQUIRE(pb_box_ok(b, field(y, 0)), MMC_ERR_ARG, "record %lld: box %g is not positive or below 2 r_cut",
                        (long long)y, field(y, 0));
        else
            MMC_REQUIRE(field(y, 0) == s.box, MMC_ERR_ARG, "record %lld: box %.17g, the batch's is %.17g", (long long)y,
                        field(y, 0), s.box);
        if (!b->temps.empty())
            MMC_REQUIRE(std::isfinite(field(y, 1)) && field(y, 1) > 0.0, MMC_ERR_ARG,
                        "record %lld: temperature %g is not positive and finite", (long long)y, field(y, 1));
    }
    if (nr > 0) {
        int64_t chunk = 0;
        MMC_TRY(state_stage(b, nr, L.bytes, &chunk));
        StateArgs a = state_args(b, L);
        const bool direct = b->state_delivery == 1; // (-1: the unpack kernel reads device staging)
        const int64_t n_chunks = (nr + chunk - 1) / chunk;
        for (int64_t c = 0; c < n_chunks; c++) { // the host fills buffer k while the kernel of chunk c - 1 reads k ^ 1
            const int k = (int)(c & 1);
            const int64_t n = std::min(chunk, nr - c * chunk);
            if (c >= 2)
                MMC_HIP(hipEventSynchronize(b->st_ev[k]));
            memcpy(b->st_h[k], in + c * chunk * L.bytes, (size_t)(n * L.bytes));
            if (!direct)
                MMC_HIP(hipMemcpyAsync(b->st_d[k], b->st_h[k], (size_t)(n * L.bytes), hipMemcpyHostToDevice, s.stream));
            a.r0 = (int)(r0 + c * chunk);
            const dim3 grid((unsigned)a.n_slabs, (unsigned)n);
            const uint8_t *src = static_cast<const uint8_t *>(direct ? b->st_hd[k] : b->st_d[k]);
            if (s.rec)
                k_state_unpack<true><<<grid, ST_BLOCK, 0, s.stream>>>(s.bv, s.rec, a, src);
            else
                k_state_unpack<false><<<grid, ST_BLOCK, 0, s.stream>>>(s.bv, s.rec, a, src);
            MMC_HIP(hipGetLastError());
            MMC_HIP(hipEventRecord(b->st_ev[k], s.stream));
        }
        s.comq_epoch++; // the candidate lists are stale
        b->cand.dirty = true;
        b->mirror_valid = false;
        MMC_TRY(s.sync());
        for (int64_t y = 0; y < nr; y++)
            b->s_cur[r0 + y] = 0; // both buffers hold S(k): the state mmc_batch_recip_long leaves
        if (s.pb.on) { // box, kappa = alpha / box, and the cfac rows and erfc tables of exactly these replicas
            std::vector<int32_t> mask(R, 0);
            for (int64_t y = 0; y < nr; y++) {
                s.pb.box[r0 + y] = field(y, 0);
                s.pb.kappa[r0 + y] = s.pb.alpha / field(y, 0);
                mask[r0 + y] = 1;
            }
            MMC_TRY(s.pb_upload_scalars());
            MMC_TRY(pb_upload_mask(s, mask));
            MMC_TRY(s.pb_build_tables(s.pb.d_mask));
            MMC_TRY(s.sync());
        }
        if (!b->temps.empty()) {
            for (int64_t y = 0; y < nr; y++)
                b->temps[r0 + y] = field(y, 1);
            MMC_TRY(tempering_upload(b));
        }
    }
    b->steps_done = info->steps_done;
    if (nr == R) {
        s.r_mol_max = info->r_mol_max;
        b->rigid_only = info->rigid_only != 0;
    } else {
        s.r_mol_max = std::max(s.r_mol_max, info->r_mol_max); // (+inf, unknown, wins)
        b->rigid_only = b->rigid_only && info->rigid_only != 0;
    }
    if (b->needs_reload) { // after a failed run: usable again once every replica has been set
        for (int64_t y = 0; y < nr; y++)
            b->reloaded[r0 + y] = 1;
        bool all = true;
        for (uint8_t v : b->reloaded) all = all && v;
        if (all) {
            b->needs_reload = false;
            b->s_cur.assign(R, 0);
        }
    }
    return MMC_OK;
}
