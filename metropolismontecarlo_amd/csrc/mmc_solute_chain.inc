// mmc_solute_chain.inc -- host side of the batch's fixed solute (include/mmc_hip.h, "A fixed solute";
// the kernels are in mmc_solute_chain.hpp): setting and reading it, its part of RecipLong and of the
// totals, and the three observables that need it (the pair energy, the radial histograms, the 3-D
// maps).  What the move driver does with it is three lines of mmc_batch.inc / mmc_engine.inc:
// batch_launch enqueues k_solute_move in front of the move kernel, and collect / mmc_batch_eval read one
// more record per move.  Included by mmc_hip.hip after mmc_units.inc, which holds the solute's record,
// refusals and parameter rows.

extern "C" int32_t mmc_batch_set_solute(mmc_batch *b, int32_t n_sites, const double *mol, const double *charge,
                                        const double *eps, const double *sig)
{
    const char *what = "mmc_batch_set_solute";
    const int32_t S = n_sites;
    MMC_REQUIRE(S >= 0 && S <= SOL_MAX_SITES, MMC_ERR_ARG, "%s: n_sites must be 0..%d (0 removes the solute)", what,
                SOL_MAX_SITES);
    const SoluteIn in{ S, nullptr, charge, eps, sig, "" };
    bool charged = false;
    double q2 = 0.0;
    if (S > 0) { // the arguments of a solute, in mmc_batch_widom_solute_at's order; none of it needs a batch
        MMC_TRY(solute_null_args(in, what));
        MMC_REQUIRE(mol, MMC_ERR_ARG, "%s: NULL mol", what);
        MMC_TRY(solute_value_args(in, what, &charged, &q2));
        for (int q = 0; q < 3 * (S + 1); q++)
            MMC_REQUIRE(std::isfinite(mol[q]), MMC_ERR_ARG, "%s: non-finite mol", what);
    }
    BATCH_CHECK(b);
    MMC_REQUIRE(!b->has_prev, MMC_ERR_STATE, "proposals outstanding: call mmc_batch_settle first");
    BATCH_NO_VOLUME_TRIAL(b);
    BatchSolute &sol = b->sol;
    DeviceSystem &s = b->sys;
    if (S > 0) {
        BATCH_ONE_BOX(b, what);
        BATCH_NOT_WOLF(b, what);
        MMC_REQUIRE(b->fast_ok, MMC_ERR_UNSUPPORTED,
                    "%s: needs identical 3-atom molecules and a cutoff / kappa the erfc table covers", what);
        if (!sol.d_par)
            MMC_TRY(s.dmalloc((void **)&sol.d_par, sizeof(double) * SOLC_PAR_DOUBLES));
        if (!sol.h_parts)
            MMC_TRY(batch_pinned((void **)&sol.h_parts, (void **)&sol.d_parts, sizeof(PartOut) * (size_t)s.R));
        double h_par[SOLC_PAR_DOUBLES] = { 0 };
        solute_pack(h_par, in, mol);
        for (int d = 0; d < 3; d++)
            h_par[SOLC_C + d] = mol[3 * S + d];
        MMC_TRY(s.sync());
        MMC_HIP(hipMemcpy(sol.d_par, h_par, sizeof(h_par), hipMemcpyHostToDevice));
    }
    // ---- nothing fails from here ----
    const bool was_charged = sol.charged;
    sol.n = S;
    sol.charged = charged;
    sol.q2 = q2;
    if (S > 0) {
        memcpy(sol.charge, charge, sizeof(double) * S);
        memcpy(sol.mol, mol, sizeof(double) * 3 * (S + 1));
        memcpy(sol.eps, eps, sizeof(double) * 3 * S);
        memcpy(sol.sig, sig, sizeof(double) * 3 * S);
    }
    sol.hash = S > 0 ? state_solute_hash(S, sol.mol, sol.charge, sol.eps, sol.sig) : 0;
    if (sol.charged || was_charged) // S(k) holds another solute's constant, or lacks this one's
        b->s_stale = true;
    return MMC_OK;
}

extern "C" int32_t mmc_batch_get_solute(mmc_batch *b, int32_t *n_sites, double *mol, double *charge, double *eps,
                                        double *sig)
{
    MMC_REQUIRE(b, MMC_ERR_ARG, "batch is NULL");
    const BatchSolute &sol = b->sol;
    if (n_sites)
        *n_sites = sol.n;
    if (mol && sol.n)
        memcpy(mol, sol.mol, sizeof(double) * 3 * (sol.n + 1));
    if (charge)
        memcpy(charge, sol.charge, sizeof(double) * sol.n);
    if (eps)
        memcpy(eps, sol.eps, sizeof(double) * 3 * sol.n);
    if (sig)
        memcpy(sig, sol.sig, sizeof(double) * 3 * sol.n);
    return MMC_OK;
}

// S(k) += S_sol(k) in both buffers of every replica, then RecipLong's energy of the sum (ewalds.jl:599):
// what mmc_batch_recip_long returns and leaves with a charged solute.  The stream is idle on entry.
static int32_t batch_solute_recip(mmc_batch *b, double *energies)
{
    DeviceSystem &s = b->sys;
    double *d_e = (double *)s.d_scr;
    k_solute_sofk<<<(unsigned)s.R, MMC_BLOCK, 0, s.stream>>>(s.bv, b->sol.view());
    k_recip_energy<<<(unsigned)s.R, MMC_BLOCK, 0, s.stream>>>(s.bv, 1, d_e);
    MMC_HIP(hipGetLastError());
    MMC_HIP(hipMemcpyAsync(energies, d_e, sizeof(double) * s.R, hipMemcpyDeviceToHost, s.stream));
    return s.sync();
}

// Workgroups of k_solute_total: one wave per replica, capped as the observables' persistent launches
// are (obs_grid: option "wave_wgs", or four waves per SIMD of every compute unit).
static unsigned solute_grid(const mmc_batch *b)
{
    return obs_grid(b, SOLC_WAVES, b->sys.R);
}

// k_solute_total of every replica into h[R][4] (raw LJ sum, raw virial sum, raw real-space sum, overlap)
static int32_t batch_solute_pairs(mmc_batch *b, std::vector<double> &h, const char *what)
{
    DeviceSystem &s = b->sys;
    const size_t R = (size_t)s.R;
    ObsCall oc(b);
    const size_t o_out = oc.take(sizeof(double) * 4 * R);
    MMC_TRY(oc.alloc());
    const PairParams pp = mmc_pair_params(b->lj_rcut, b->qq_rcut, 0.0, 0.5, s.bv.kappa, false);
    k_solute_total<<<solute_grid(b), SOLC_WAVES * 64, 0, oc.st>>>(
        s.bv, s.rec, b->sol.view(), s.qq_tab, s.fc, pp, oc.at<double>(o_out), (int)R);
    oc.launched();
    h.resize(4 * R);
    oc.to_host(h.data(), oc.at<double>(o_out), sizeof(double) * 4 * R);
    return oc.finish(what);
}

// The solute's part of potential(..., "ewald") of the N + 1 system (energy.jl:946-1032), put into the
// sums DeviceSystem::totals_ewald forms the totals from: each water-solute pair is in the reference's
// double-counted sums twice -- once with the water chosen, once with the solute -- S(k) and its energy
// are those of all N + 1 molecules, and EwaldSelf runs over the solute's charges too.
struct SoluteTotalsCtx {
    mmc_batch *b;
    std::vector<uint8_t> ovl;
};
static int32_t solute_totals_hook(void *ctx_, std::vector<TotalsRaw> &ht, std::vector<double> &erec, double *sq2)
{
    SoluteTotalsCtx *ctx = static_cast<SoluteTotalsCtx *>(ctx_);
    mmc_batch *b = ctx->b;
    const int64_t R = b->sys.R;
    std::vector<double> h;
    MMC_TRY(batch_solute_pairs(b, h, "mmc_batch_potential_ewald"));
    if (b->sol.charged)
        MMC_TRY(batch_solute_recip(b, erec.data()));
    ctx->ovl.assign((size_t)R, 0);
    for (int64_t r = 0; r < R; r++) {
        const double *o = &h[4 * (size_t)r];
        const double e = (0.0 + o[0]) * 4, v = (0.0 + o[1]) * 24 / 3.0; // energy.jl:289 (mmc_combine_parts)
        ht[r].lj_e += e + e;
        ht[r].lj_v += v + v;
        ht[r].qq += o[2] + o[2];
        ctx->ovl[r] = o[3] != 0.0;
    }
    *sq2 += b->sol.q2;
    return MMC_OK;
}

static int32_t batch_solute_totals(mmc_batch *b, mmc_totals *tot)
{
    SoluteTotalsCtx ctx{ b, {} };
    const TotalsHook hook{ &solute_totals_hook, &ctx };
    MMC_TRY(b->sys.totals_ewald(b->lj_rcut, b->qq_rcut, tot, &hook));
    for (int64_t r = 0; r < b->sys.R; r++)
        if (ctx.ovl[r]) { // (as with per-replica boxes: the reference's EwaldReal would return (0.0, true) for the pair)
            tot[r].energy = INFINITY;
            tot[r].n_overlap += 1;
        }
    return MMC_OK;
}

extern "C" int32_t mmc_batch_solute_energy(mmc_batch *b, double *u_lj, double *u_real, uint8_t *ovl)
{
    const char *what = "mmc_batch_solute_energy";
    MMC_REQUIRE(u_lj && u_real && ovl, MMC_ERR_ARG, "%s: NULL out pointer", what);
    BATCH_CHECK(b);
    STRUCT_STATE(b);
    MMC_REQUIRE(b->sol.n > 0, MMC_ERR_STATE, "%s: no solute is set (mmc_batch_set_solute)", what);
    std::vector<double> h;
    MMC_TRY(batch_solute_pairs(b, h, what));
    for (int64_t r = 0; r < b->sys.R; r++) {
        const double *o = &h[4 * (size_t)r];
        const bool ov = o[3] != 0.0;
        u_lj[r] = (0.0 + o[0]) * 4;            // energy.jl:289
        double real = ov ? 0.0 : 0.0 + o[2];   // ewalds.jl:359-360
        real *= b->sys.bv.factor;              // ewalds.jl:905
        u_real[r] = real;
        ovl[r] = ov ? 1 : 0;
    }
    return MMC_OK;
}

extern "C" int32_t mmc_batch_rdf_solute(mmc_batch *b, int32_t numbins, double r_max, int32_t per_replica,
                                        uint64_t *hist)
{
    const char *what = "mmc_batch_rdf_solute";
    MMC_REQUIRE(hist, MMC_ERR_ARG, "%s: NULL out pointer", what);
    MMC_REQUIRE(numbins >= 1 && numbins <= MMC_RDF_SITES_MAX_BINS, MMC_ERR_ARG, "%s: numbins outside 1..%d", what,
                MMC_RDF_SITES_MAX_BINS);
    MMC_REQUIRE(std::isfinite(r_max), MMC_ERR_ARG, "%s: r_max is not finite", what);
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    TileArgs ta{};
    std::vector<double> thr;
    MMC_TRY(tile_plan(b, numbins, r_max, what, &ta, &thr)); // (the range, the state, dr and its thresholds)
    MMC_REQUIRE(b->sol.n > 0, MMC_ERR_STATE, "%s: no solute is set (mmc_batch_set_solute)", what);
    const size_t R = (size_t)s.R;
    const size_t hist_bytes = sizeof(unsigned long long) * (per_replica ? R : 1) * (size_t)(1 + b->sol.n) * 3 * (size_t)numbins;
    ObsCall oc(b);
    const size_t o_hist = oc.take(hist_bytes), o_thr = oc.take(sizeof(double) * thr.size());
    MMC_TRY(oc.alloc());
    RdfSoluteArgs ra{};
    ra.thr = oc.at<double>(o_thr);
    ra.hist = oc.at<unsigned long long>(o_hist);
    ra.numbins = numbins;
    ra.per_replica = per_replica ? 1 : 0;
    ra.inv_dr = ta.inv_dr;
    ra.R = (int32_t)R;
    oc.zero(hist_bytes);
    oc.to_device(oc.at<double>(o_thr), thr.data(), sizeof(double) * thr.size());
    if (oc.e == hipSuccess)
        k_rdf_solute<<<obs_grid(b, SOLC_WAVES, (int64_t)R * SOLC_WAVES), SOLC_WAVES * 64, sizeof(unsigned) * 3 * (size_t)numbins, oc.st>>>(
            s.bv, s.rec, b->sol.view(), ra); // (a workgroup per replica; 12 numbins <= 24 KiB of LDS)
    oc.launched();
    oc.fetch(hist, ra.hist, hist_bytes);
    return oc.finish(what);
}

extern "C" int32_t mmc_batch_hydration_map(mmc_batch *b, int32_t n_half, double cell, int32_t channel_mask,
                                           int32_t per_replica, int64_t *maps)
{
    const char *what = "mmc_batch_hydration_map";
    // what can be refused without the batch comes first
    MMC_REQUIRE(maps, MMC_ERR_ARG, "%s: NULL out pointer", what);
    MMC_REQUIRE(n_half >= 1, MMC_ERR_ARG, "%s: n_half must be >= 1", what);
    MMC_REQUIRE(std::isfinite(cell) && cell > 0.0, MMC_ERR_ARG, "%s: cell must be finite and > 0", what);
    MMC_REQUIRE(channel_mask >= 1 && channel_mask < (1 << MMC_HMAP_CHANNELS), MMC_ERR_ARG, "%s: channel_mask outside 1..%d",
                what, (1 << MMC_HMAP_CHANNELS) - 1);
    MMC_REQUIRE(n_half <= 12 && 8 * (int64_t)n_half * n_half * n_half <= MMC_HMAP_MAX_CELLS, MMC_ERR_ARG,
                "%s: the grid has more than %d cells", what, MMC_HMAP_MAX_CELLS);
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    STRUCT_STATE(b);
    MMC_REQUIRE(b->sol.n > 0, MMC_ERR_STATE, "%s: no solute is set (mmc_batch_set_solute)", what);
    // (one box and Ewald style: mmc_batch_set_solute fences the rest)
    MMC_REQUIRE(!((double)n_half * cell > s.bv.box / 2.0), MMC_ERR_ARG,
                "%s: n_half cell = %g exceeds half of the box %g: the cube would reach a second image", what,
                (double)n_half * cell, s.bv.box);
    const int n_edge = 2 * n_half + 1;
    const int64_t n_cells = 8 * (int64_t)n_half * n_half * n_half;
    const size_t lds = 8 * (size_t)n_edge + 8 * (size_t)n_cells;
    MMC_REQUIRE((int64_t)lds + 64 <= s.lds_per_block, MMC_ERR_UNSUPPORTED,
                "%s: the device grants %lld bytes of LDS per workgroup, %lld cells need %zu", what,
                (long long)s.lds_per_block, (long long)n_cells, lds + 64);
    // (holds while a solute is set: mmc_batch_set_solute requires fast_ok of a homogeneous batch, and what
    // could clear it -- a volume change, per-replica boxes, Wolf style -- is fenced)
    MMC_REQUIRE(struct_use_rec(b), MMC_ERR_UNSUPPORTED, "%s: the batch does not keep its molecules' records in step", what);
    std::vector<double> edge((size_t)n_edge);
    for (int k = -n_half; k <= n_half; k++)
        edge[(size_t)(k + n_half)] = (double)k * cell;

    const size_t R = (size_t)s.R;
    const size_t n_ch = (size_t)__builtin_popcount((unsigned)channel_mask);
    const size_t map_bytes = sizeof(unsigned long long) * (per_replica ? R : 1) * n_ch * (size_t)(n_cells + 2);
    ObsCall oc(b);
    const size_t o_maps = oc.take(map_bytes), o_edge = oc.take(sizeof(double) * edge.size());
    MMC_TRY(oc.alloc()); // (the per-replica output in one piece: the allocation's status if the device has no room)
    HmapArgs ha{};
    ha.edge = oc.at<double>(o_edge);
    ha.maps = oc.at<unsigned long long>(o_maps);
    ha.n_half = n_half;
    ha.n_cells = (int32_t)n_cells;
    ha.channel_mask = channel_mask;
    ha.per_replica = per_replica ? 1 : 0;
    ha.inv_cell = (float)(1.0 / cell);
    ha.R = (int32_t)R;
    const PairParams pp = mmc_pair_params(b->lj_rcut, b->qq_rcut, 0.0, 0.5, s.bv.kappa, false);
    if (lds > TILE_LDS_BYTES) // beyond what a workgroup may ask for without opting in: as k_sdf_wave
        oc.e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_hydration_map), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)(s.lds_per_block - 64));
    oc.zero(map_bytes);
    oc.to_device(oc.at<double>(o_edge), edge.data(), sizeof(double) * edge.size());
    // one workgroup of sixteen waves per compute unit (its grid may take 128 KB of the unit's LDS), a replica at a time
    const unsigned wgs = obs_grid(b, HMAP_THREADS / 64, (int64_t)R * (HMAP_THREADS / 64));
    if (oc.e == hipSuccess)
        k_hydration_map<<<wgs, HMAP_THREADS, lds, oc.st>>>(s.bv, s.rec, b->sol.view(), s.qq_tab, s.fc, pp, ha);
    oc.launched();
    oc.fetch(maps, ha.maps, map_bytes);
    return oc.finish(what);
}
