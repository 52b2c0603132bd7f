// mmc_perbox.inc -- independent NPT replicas in one batch: a box per replica (include/mmc_hip.h,
// "Per-replica boxes").  Replica r has its own L_r, kappa_r = alpha / L_r (Ewald/main.jl:290-291),
// cfac row and erfc table (DeviceSystem::pb); trial moves run on k_propose and k_move_eval_fast with
// a PerBoxView, totals and RecipLong on the per-box paths of DeviceSystem, and a volume move of any
// subset of the replicas is one batched trial (k_rescale_pb, k_cfac_pb, k_build_qq_table with a
// PerBoxTable, potential()) and one settle (k_copy_replicas over every replica not accepted).
// Included by mmc_hip.hip after mmc_engine.inc.

// The erfc table holds for kappa * sqrt(r_cut^2 + 100) <= MMC_QQ_XMAX and kappa <= MMC_QQ_KAPPA_MAX
// (DeviceSystem::fast_table_ok); kappa = alpha / L grows as the box shrinks, so the whole chain is
// covered when the smallest box a volume move admits, L = 2 r_cut, is.
static bool pb_domain_ok(const mmc_batch *b, double alpha)
{
    const DeviceSystem &s = b->sys;
    const double rc = std::max(b->lj_rcut, b->qq_rcut);
    const double kappa = alpha / (2.0 * rc), slack = b->qq_rcut * b->qq_rcut + 100; // ewalds.jl:362
    return s.homogeneous && s.rec && s.n_mol <= MMC_WAVE_MAX_MOL && kappa <= MMC_QQ_KAPPA_MAX &&
           slack <= MMC_QQ_UMAX && kappa * std::sqrt(slack) <= MMC_QQ_XMAX;
}

static bool pb_box_ok(const mmc_batch *b, double L)
{
    return std::isfinite(L) && L > 0 && b->lj_rcut <= L / 2 && b->qq_rcut <= L / 2;
}

static int32_t pb_upload_mask(DeviceSystem &s, const std::vector<int32_t> &mask)
{
    MMC_HIP(hipMemcpyAsync(s.pb.d_mask, mask.data(), sizeof(int32_t) * s.R, hipMemcpyHostToDevice, s.stream));
    return s.sync();
}

#define PB_DOMAIN_MSG                                                                            \
    "per-replica boxes: the erfc table does not cover kappa = alpha / (2 r_cut) = %.4g (needs "  \
    "kappa <= %.2f and kappa * sqrt(r_cut^2 + 100) <= %.1f, identical 3-atom molecules, at most %d)"

extern "C" int32_t mmc_batch_set_boxes(mmc_batch *b, const double *boxes, double alpha)
{
    BATCH_CHECK(b);
    BATCH_NOT_WOLF(b, "mmc_batch_set_boxes");
    BATCH_NO_SOLUTE(b, "mmc_batch_set_boxes");
    BATCH_USABLE(b);
    BATCH_NO_VOLUME_TRIAL(b);
    MMC_REQUIRE(boxes, MMC_ERR_ARG, "NULL argument");
    MMC_REQUIRE(!b->has_prev, MMC_ERR_STATE, "proposals outstanding: call mmc_batch_settle first");
    MMC_REQUIRE(alpha > 0 && std::isfinite(alpha), MMC_ERR_ARG, "alpha must be positive");
    DeviceSystem &s = b->sys;
    const int64_t R = s.R;
    for (int64_t r = 0; r < R; r++)
        MMC_REQUIRE(pb_box_ok(b, boxes[r]), MMC_ERR_ARG,
                    "replica %lld: box %g is not positive or below 2 r_cut", (long long)r, boxes[r]);
    MMC_REQUIRE(pb_domain_ok(b, alpha), MMC_ERR_UNSUPPORTED, PB_DOMAIN_MSG,
                alpha / (2.0 * std::max(b->lj_rcut, b->qq_rcut)), MMC_QQ_KAPPA_MAX, MMC_QQ_XMAX,
                MMC_WAVE_MAX_MOL);
    MMC_REQUIRE(!b->quat_mode, MMC_ERR_UNSUPPORTED,
                "per-replica boxes: orientations (mmc_batch_set_orientations) are not supported");
    MMC_REQUIRE(b->persistent != 1, MMC_ERR_UNSUPPORTED,
                "per-replica boxes: the move server has one box (option persistent = 1)");
    if (!s.pb.d_box) {
        MMC_TRY(s.dmalloc((void **)&s.pb.d_box, sizeof(double) * R));
        MMC_TRY(s.dmalloc((void **)&s.pb.d_kappa, sizeof(double) * R));
        MMC_TRY(s.dmalloc((void **)&s.pb.d_f, sizeof(double) * R));
        MMC_TRY(s.dmalloc((void **)&s.pb.d_new_box, sizeof(double) * R));
        MMC_TRY(s.dmalloc((void **)&s.pb.cfac, sizeof(double) * MMC_NK_STRIDE * R));
        MMC_TRY(s.dmalloc((void **)&s.pb.tab, sizeof(double) * MMC_QQ_TABLE_DOUBLES * R));
        MMC_TRY(s.dmalloc((void **)&s.pb.d_mask, sizeof(int32_t) * R));
        MMC_HIP(hipMemsetAsync(s.pb.cfac, 0, sizeof(double) * MMC_NK_STRIDE * R, s.stream));
    }
    s.pb.box.assign(boxes, boxes + R);
    s.pb.kappa.resize(R);
    for (int64_t r = 0; r < R; r++)
        s.pb.kappa[r] = alpha / boxes[r];
    s.pb.alpha = alpha;
    MMC_TRY(s.pb_upload_scalars());
    MMC_TRY(s.pb_build_tables(nullptr));
    MMC_TRY(s.sync());
    s.pb.on = true;
    b->device_moves = 1;      // (k_propose with a PerBoxView: the moves are drawn on the device)
    b->mirror_valid = false;
    b->fast_ok = true;
    return MMC_OK;
}

extern "C" int32_t mmc_batch_get_boxes(mmc_batch *b, double *boxes)
{
    BATCH_CHECK(b);
    MMC_REQUIRE(boxes, MMC_ERR_ARG, "NULL argument");
    for (int64_t r = 0; r < b->sys.R; r++)
        boxes[r] = b->sys.pb.on ? b->sys.pb.box[r] : b->sys.box;
    return MMC_OK;
}

extern "C" int32_t mmc_batch_volume_trial_replicas(mmc_batch *b, const double *new_boxes, mmc_totals *tot)
{
    BATCH_CHECK(b);
    BATCH_NOT_WOLF(b, "mmc_batch_volume_trial_replicas");
    BATCH_USABLE(b);
    BATCH_NO_VOLUME_TRIAL(b);
    MMC_REQUIRE(new_boxes && tot, MMC_ERR_ARG, "NULL argument");
    MMC_REQUIRE(!b->has_prev, MMC_ERR_STATE, "proposals outstanding: call mmc_batch_settle first");
    DeviceSystem &s = b->sys;
    MMC_REQUIRE(s.pb.on, MMC_ERR_UNSUPPORTED,
                "mmc_batch_volume_trial_replicas needs per-replica boxes (mmc_batch_set_boxes)");
    const int64_t R = s.R;
    for (int64_t r = 0; r < R; r++)
        MMC_REQUIRE(new_boxes[r] == 0.0 || pb_box_ok(b, new_boxes[r]), MMC_ERR_ARG,
                    "replica %lld: new box %g is not positive or below 2 r_cut", (long long)r, new_boxes[r]);
    // every replica is copied aside: a replica that does not move keeps its coordinates, but the
    // total energy below recomputes its S(k), which the settle gives back bit for bit
    MMC_TRY(pb_upload_mask(s, std::vector<int32_t>(R, 1)));
    MMC_TRY(s.pb_snapshot(s.pb.d_mask, true));
    s.pb.snap_box = s.pb.box;
    s.pb.snap_kappa = s.pb.kappa;
    std::vector<double> f(R), nb(R);
    std::vector<int32_t> moved(R);
    for (int64_t r = 0; r < R; r++) {
        moved[r] = new_boxes[r] != 0.0;
        f[r] = moved[r] ? new_boxes[r] / s.pb.box[r] : 0.0; // (mmc_batch_volume_change's arithmetic)
        nb[r] = moved[r] ? new_boxes[r] : s.pb.box[r];
        if (moved[r]) {
            s.pb.box[r] = new_boxes[r];
            s.pb.kappa[r] = s.pb.alpha / new_boxes[r];
        }
    }
    MMC_HIP(hipMemcpyAsync(s.pb.d_f, f.data(), sizeof(double) * R, hipMemcpyHostToDevice, s.stream));
    MMC_HIP(hipMemcpyAsync(s.pb.d_new_box, nb.data(), sizeof(double) * R, hipMemcpyHostToDevice, s.stream));
    MMC_TRY(s.sync()); // (pageable host arrays)
    MMC_TRY(pb_upload_mask(s, moved));
    dim3 grid((unsigned)((s.n_mol + 255) / 256), (unsigned)R);
    k_rescale_pb<<<grid, 256, 0, s.stream>>>(s.bv, s.rec, s.pb.d_f, s.pb.d_new_box); // volumeChange.jl:62-80
    s.comq_epoch++;
    MMC_HIP(hipGetLastError());
    MMC_TRY(s.pb_upload_scalars());
    MMC_TRY(s.pb_build_tables(s.pb.d_mask));            // ewalds.jl:45-103 for alpha / L_new
    b->mirror_valid = false;
    int32_t st = s.totals_ewald(b->lj_rcut, b->qq_rcut, tot); // volumeChange.jl:91-111
    if (st != MMC_OK) { // leave the batch as it was
        (void)pb_upload_mask(s, std::vector<int32_t>(R, 1));
        (void)s.pb_snapshot(s.pb.d_mask, false);
        s.pb.box = s.pb.snap_box;
        s.pb.kappa = s.pb.snap_kappa;
        (void)s.pb_upload_scalars();
        return st;
    }
    b->pb_moved = moved;
    b->vol_outstanding = true;
    return MMC_OK;
}

extern "C" int32_t mmc_batch_volume_settle(mmc_batch *b, const int32_t *accept)
{
    BATCH_CHECK(b);
    BATCH_NOT_WOLF(b, "mmc_batch_volume_settle");
    MMC_REQUIRE(accept, MMC_ERR_ARG, "NULL argument");
    DeviceSystem &s = b->sys;
    MMC_REQUIRE(s.pb.on, MMC_ERR_UNSUPPORTED,
                "mmc_batch_volume_settle needs per-replica boxes (mmc_batch_set_boxes)");
    MMC_REQUIRE(b->vol_outstanding, MMC_ERR_STATE, "no volume move outstanding");
    const int64_t R = s.R;
    std::vector<int32_t> restore(R);
    for (int64_t r = 0; r < R; r++) {
        restore[r] = !(b->pb_moved[r] && accept[r]);
        if (restore[r]) {
            s.pb.box[r] = s.pb.snap_box[r];
            s.pb.kappa[r] = s.pb.snap_kappa[r];
        }
    }
    MMC_TRY(pb_upload_mask(s, restore));
    MMC_TRY(s.pb_snapshot(s.pb.d_mask, false)); // one launch over every replica given back
    MMC_TRY(s.pb_upload_scalars());
    b->vol_outstanding = false;
    return MMC_OK;
}

// mmc_batch_run_npt's chain for every replica of a batch with per-replica boxes: n_sweeps x { a
// sweep of trial moves for all replicas (mmc_batch_run), one batched volume move }.
extern "C" int32_t mmc_batch_run_npt_replicas(mmc_batch *b, const mmc_run_params *p, const mmc_npt_params *q,
                                              const double *pressures, double *energies,
                                              mmc_run_stats *stats, mmc_npt_stats *per_replica)
{
    BATCH_CHECK(b);
    BATCH_NOT_WOLF(b, "mmc_batch_run_npt_replicas");
    MMC_REQUIRE(p && q && energies && stats && per_replica, MMC_ERR_ARG, "NULL argument");
    DeviceSystem &s = b->sys;
    MMC_REQUIRE(s.pb.on, MMC_ERR_UNSUPPORTED,
                "mmc_batch_run_npt_replicas needs per-replica boxes (mmc_batch_set_boxes)");
    MMC_REQUIRE(q->n_sweeps >= 0 && q->moves_per_sweep >= 0 && q->vmax >= 0 && q->alpha > 0
                    && p->temperature > 0, MMC_ERR_ARG, "bad NPT parameters");
    MMC_REQUIRE(pb_domain_ok(b, q->alpha), MMC_ERR_UNSUPPORTED, PB_DOMAIN_MSG,
                q->alpha / (2.0 * std::max(b->lj_rcut, b->qq_rcut)), MMC_QQ_KAPPA_MAX, MMC_QQ_XMAX,
                MMC_WAVE_MAX_MOL);
    MMC_REQUIRE(q->alpha == s.pb.alpha, MMC_ERR_ARG,
                "alpha %g differs from the one the boxes were set with (%g)", q->alpha, s.pb.alpha);
    const int64_t R = s.R, n_mol = s.n_mol;
    memset(stats, 0, sizeof(*stats));
    memset(per_replica, 0, sizeof(mmc_npt_stats) * R);
    mmc_run_params pp = *p;
    pp.n_steps = q->moves_per_sweep > 0 ? q->moves_per_sweep : n_mol;
    std::vector<double> new_boxes(R), vol_new(R), u_b(R);
    std::vector<mmc_totals> tot(R);
    std::vector<int32_t> accept(R);
    for (int64_t sweep = 0; sweep < q->n_sweeps; sweep++) {
        mmc_run_stats st;
        MMC_TRY(run_impl(b, &pp, energies, nullptr, 0, &st));
        stats->moves += st.moves; stats->launches += st.launches;
        stats->trans_attempt += st.trans_attempt; stats->trans_accept += st.trans_accept;
        stats->rot_attempt += st.rot_attempt; stats->rot_accept += st.rot_accept;
        stats->overlaps += st.overlaps; stats->kernel_ms += st.kernel_ms;
        stats->timed_launches += st.timed_launches; stats->torn_records += st.torn_records;
        stats->server_steps += st.server_steps; stats->wall_ms += st.wall_ms;
        stats->device_decisions += st.device_decisions;
        // ---- one volume move per replica, all in one batched trial ----
        const auto t0 = std::chrono::steady_clock::now();
        bool any = false;
        for (int64_t r = 0; r < R; r++) {
            const ChainKey ck{ p->seed, (uint32_t)(p->replica0 + (uint64_t)r) };
            const Uniform2 u = mmc_draw(ck, (uint64_t)b->steps_done, MMC_SLOT_VOLUME);
            const double box = s.pb.box[r], vol_old = box * box * box;
            vol_new[r] = vol_old + (u.a - 0.5) * q->vmax;                  // volumeChange.jl:59
            u_b[r] = u.b;
            new_boxes[r] = 0.0;
            per_replica[r].vol_attempt++;
            if (vol_new[r] > 0.0) {
                const double L_new = cbrt(vol_new[r]);                     // :60
                if (b->lj_rcut <= L_new / 2 && b->qq_rcut <= L_new / 2)    // (else: minimum image would break)
                    new_boxes[r] = L_new;
            }
            any = any || new_boxes[r] != 0.0;
        }
        if (any) {
            std::vector<double> vol_old(R);
            for (int64_t r = 0; r < R; r++)
                vol_old[r] = s.pb.box[r] * s.pb.box[r] * s.pb.box[r];
            MMC_TRY(mmc_batch_volume_trial_replicas(b, new_boxes.data(), tot.data()));
            for (int64_t r = 0; r < R; r++) {
                accept[r] = 0;
                if (new_boxes[r] == 0.0)
                    continue;
                const double P = pressures ? pressures[r] : q->pressure;
                // (re-read every sweep: the caller's exchanges between calls permute the temperatures)
                const double beta = 1.0 / (b->temps.empty() ? p->temperature : b->temps[r]);
                const double arg = -beta * (P * (vol_new[r] - vol_old[r])
                                            - (double)n_mol * log(vol_new[r] / vol_old[r]) / beta
                                            + (tot[r].energy - energies[r])); // :129-130
                accept[r] = u_b[r] < exp(arg < 700.0 ? arg : 700.0);          // :132
                if (accept[r]) {
                    energies[r] = tot[r].energy;
                    per_replica[r].vol_accept++;
                }
            }
            MMC_TRY(mmc_batch_volume_settle(b, accept.data()));
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        for (int64_t r = 0; r < R; r++) {
            const double L = s.pb.box[r];
            per_replica[r].volume_sum += L * L * L;
            per_replica[r].volume_ms += ms;
        }
    }
    for (int64_t r = 0; r < R; r++) {
        per_replica[r].box = s.pb.box[r];
        stats->energy_sum += energies[r];
    }
    return MMC_OK;
}
