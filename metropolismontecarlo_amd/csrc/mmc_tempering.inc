// mmc_tempering.inc -- parallel tempering on the replica batch (include/mmc_hip.h, "Parallel
// tempering"): a temperature per replica, read by every accept decision (Driver::decide on the host,
// wave_decide<true> in the LADDER forms of k_move_eval_wave, the volume criterion of
// mmc_batch_run_npt_replicas), and ladder exchanges decided by a pure host function.  A swap
// exchanges temperatures, never configurations: coordinates, S(k) buffers, records and flag bytes
// stay where they are.  Included by mmc_hip.hip after mmc_perbox.inc.

// The batch's temperatures to the device array the LADDER kernels read (DecideConsts::temps).
// No launch of a preceding run can still read it: run_impl returns only after it has synchronised
// every group's stream, and the last thing it enqueues there, the commit of the final accepted
// moves, takes no DecideConsts at all.  Callers are refused while proposals are outstanding or a
// volume trial is open, so nothing of mmc_batch_eval's is in flight either.  hipMemcpy from pageable
// memory has completed when it returns, before the next run's first launch is enqueued.
static int32_t tempering_upload(mmc_batch *b)
{
    if (b->temps.empty())
        return MMC_OK;
    if (!b->d_temps)
        MMC_TRY(b->sys.dmalloc((void **)&b->d_temps, sizeof(double) * b->sys.R));
    MMC_HIP(hipMemcpy(b->d_temps, b->temps.data(), sizeof(double) * b->sys.R, hipMemcpyHostToDevice));
    return MMC_OK;
}

#define BATCH_BETWEEN_MOVES(b)                                                                   \
    MMC_REQUIRE(!(b)->has_prev, MMC_ERR_STATE, "proposals outstanding: call mmc_batch_settle first"); \
    BATCH_NO_VOLUME_TRIAL(b)

extern "C" int32_t mmc_batch_set_temperatures(mmc_batch *b, const double *temps)
{
    BATCH_CHECK(b);
    BATCH_BETWEEN_MOVES(b);
    const int64_t R = b->sys.R;
    if (!temps) {
        b->temps.clear();
        return MMC_OK;
    }
    for (int64_t r = 0; r < R; r++)
        MMC_REQUIRE(std::isfinite(temps[r]) && temps[r] > 0.0, MMC_ERR_ARG,
                    "replica %lld: temperature %g is not positive and finite", (long long)r, temps[r]);
    const std::vector<double> before = b->temps;
    b->temps.assign(temps, temps + R);
    const int32_t st = tempering_upload(b);
    if (st != MMC_OK)
        b->temps = before;
    return st;
}

extern "C" int32_t mmc_batch_get_temperatures(mmc_batch *b, double *temps)
{
    BATCH_CHECK(b);
    MMC_REQUIRE(temps, MMC_ERR_ARG, "NULL argument");
    for (int64_t r = 0; r < b->sys.R; r++)
        temps[r] = b->temps.empty() ? 0.0 : b->temps[r];
    return MMC_OK;
}

// What mmc_exchange_round refuses, checked before anything is changed; holder[l n_rungs + k] = the
// replica of ladder l that holds rung k.
static int32_t exchange_check(int64_t n_ladders, int32_t n_rungs, int32_t parity, const double *temps,
                              const int32_t *rung, std::vector<int64_t> &holder)
{
    MMC_REQUIRE(n_ladders >= 1, MMC_ERR_ARG, "n_ladders must be >= 1");
    MMC_REQUIRE(n_rungs >= 2, MMC_ERR_ARG, "n_rungs must be >= 2: a ladder of %d has no pair to exchange", (int)n_rungs);
    MMC_REQUIRE(parity == 0 || parity == 1, MMC_ERR_ARG, "parity must be 0 or 1, not %d", (int)parity);
    MMC_REQUIRE(temps && rung, MMC_ERR_ARG, "NULL argument");
    holder.assign((size_t)(n_ladders * n_rungs), -1);
    for (int64_t r = 0; r < n_ladders * n_rungs; r++) {
        MMC_REQUIRE(std::isfinite(temps[r]) && temps[r] > 0.0, MMC_ERR_ARG,
                    "replica %lld: temperature %g is not positive and finite", (long long)r, temps[r]);
        const int64_t l = r / n_rungs;
        MMC_REQUIRE(rung[r] >= 0 && rung[r] < n_rungs && holder[(size_t)(l * n_rungs + rung[r])] < 0, MMC_ERR_ARG,
                    "rung is not a permutation of 0..%d within ladder %lld (replica %lld holds %d)",
                    (int)n_rungs - 1, (long long)l, (long long)r, (int)rung[r]);
        holder[(size_t)(l * n_rungs + rung[r])] = r;
    }
    return MMC_OK;
}

extern "C" int32_t mmc_exchange_round(int64_t n_ladders, int32_t n_rungs, int32_t parity, uint64_t seed,
                                      uint64_t replica0, uint64_t round, double pressure,
                                      const double *energies, const double *volumes, double *temps,
                                      int32_t *rung, int64_t *attempt, int64_t *accept)
{
    MMC_REQUIRE(energies && attempt && accept, MMC_ERR_ARG, "NULL argument");
    std::vector<int64_t> holder;
    MMC_TRY(exchange_check(n_ladders, n_rungs, parity, temps, rung, holder));
    for (int64_t l = 0; l < n_ladders; l++)
        for (int32_t k = parity; k + 1 < n_rungs; k += 2) {
            const int64_t a = holder[(size_t)(l * n_rungs + k)], c = holder[(size_t)(l * n_rungs + k + 1)];
            attempt[k]++;
            double dw = energies[a] - energies[c];
            if (volumes)
                dw = dw + pressure * (volumes[a] - volumes[c]);
            const double D = (1.0 / temps[a] - 1.0 / temps[c]) * dw;
            const double u = mmc_draw(ChainKey{ seed, (uint32_t)(replica0 + (uint64_t)(l * n_rungs + k)) }, round,
                                      MMC_SLOT_EXCHANGE).a;
            if (!(std::isfinite(energies[a]) && std::isfinite(energies[c]) && std::isfinite(D)))
                continue; // (an overlapping start carries +inf: it never swaps)
            if (D >= 0.0 || u < std::exp(D)) {
                std::swap(temps[a], temps[c]);
                std::swap(rung[a], rung[c]);
                accept[k]++;
            }
        }
    return MMC_OK;
}

// The exchange on the batch's own array; `holder` is scratch.
static int32_t batch_exchange_checked(mmc_batch *b, int32_t n_rungs, int32_t parity, uint64_t seed, uint64_t replica0,
                                      uint64_t round, double pressure, const double *energies, int32_t *rung,
                                      int64_t *attempt, int64_t *accept)
{
    const int64_t R = b->sys.R;
    std::vector<double> vol;
    if (b->sys.pb.on) {
        vol.resize(R);
        for (int64_t r = 0; r < R; r++)
            vol[r] = b->sys.pb.box[r] * b->sys.pb.box[r] * b->sys.pb.box[r];
    }
    MMC_TRY(mmc_exchange_round(R / n_rungs, n_rungs, parity, seed, replica0, round, pressure, energies,
                               vol.empty() ? nullptr : vol.data(), b->temps.data(), rung, attempt, accept));
    return tempering_upload(b);
}

#define BATCH_LADDERS(b, n_rungs)                                                                \
    MMC_REQUIRE(!(b)->temps.empty(), MMC_ERR_STATE,                                              \
                "no per-replica temperatures: call mmc_batch_set_temperatures first");           \
    MMC_REQUIRE((n_rungs) >= 2 && (b)->sys.R % (n_rungs) == 0, MMC_ERR_ARG,                      \
                "%lld replicas are not whole ladders of %d rungs (n_rungs >= 2)", (long long)(b)->sys.R, (int)(n_rungs))

extern "C" int32_t mmc_batch_exchange(mmc_batch *b, int32_t n_rungs, int32_t parity, uint64_t seed, uint64_t replica0,
                                      uint64_t round, double pressure, const double *energies, int32_t *rung,
                                      int64_t *attempt, int64_t *accept)
{
    BATCH_CHECK(b);
    BATCH_BETWEEN_MOVES(b);
    BATCH_LADDERS(b, n_rungs);
    return batch_exchange_checked(b, n_rungs, parity, seed, replica0, round, pressure, energies, rung, attempt, accept);
}

extern "C" int32_t mmc_batch_run_exchange(mmc_batch *b, const mmc_run_params *p, int64_t n_rounds, int32_t n_rungs,
                                          uint64_t round0, double *energies, int32_t *rung, int64_t *attempt,
                                          int64_t *accept, mmc_run_stats *stats)
{
    BATCH_CHECK(b);
    BATCH_ONE_BOX(b, "mmc_batch_run_exchange (an NPT ladder: mmc_batch_run_npt_replicas of one sweep, then mmc_batch_exchange)");
    BATCH_BETWEEN_MOVES(b);
    MMC_REQUIRE(p && energies && rung && attempt && accept && stats, MMC_ERR_ARG, "NULL argument");
    MMC_REQUIRE(n_rounds >= 0, MMC_ERR_ARG, "n_rounds must be >= 0");
    BATCH_LADDERS(b, n_rungs);
    {   // (the exchange's arguments, before the first move)
        std::vector<int64_t> holder;
        MMC_TRY(exchange_check(b->sys.R / n_rungs, n_rungs, 0, b->temps.data(), rung, holder));
    }
    memset(stats, 0, sizeof(*stats));
    for (int64_t i = 0; i < n_rounds; i++) {
        mmc_run_stats st;
        MMC_TRY(run_impl(b, p, energies, nullptr, 0, &st));
        stats->moves += st.moves; stats->launches += st.launches;
        stats->trans_attempt += st.trans_attempt; stats->trans_accept += st.trans_accept;
        stats->rot_attempt += st.rot_attempt; stats->rot_accept += st.rot_accept;
        stats->overlaps += st.overlaps; stats->kernel_ms += st.kernel_ms;
        stats->timed_launches += st.timed_launches; stats->torn_records += st.torn_records;
        stats->server_steps += st.server_steps; stats->wall_ms += st.wall_ms;
        stats->device_decisions += st.device_decisions;
        const uint64_t round = round0 + (uint64_t)i;
        MMC_TRY(batch_exchange_checked(b, n_rungs, (int32_t)(round & 1), p->seed, p->replica0, round, 0.0, energies,
                                       rung, attempt, accept));
    }
    for (int64_t r = 0; r < b->sys.R; r++)
        stats->energy_sum += energies[r];
    return MMC_OK;
}
