// mmc_cavity.inc -- host side of mmc_batch_cavity and mmc_batch_cavity_at (include/mmc_hip.h,
// "Cavities and occupancy"; the kernel is in mmc_cavity.hpp).  Included by mmc_hip.hip after
// mmc_units.inc (ObsCall).
#include "mmc_cavity.hpp"

static int32_t cavity_run(mmc_batch *b, int64_t n_probe, uint64_t seed, int64_t draw0, const double *points_in,
                          bool at, int32_t site, int32_t n_radii, const double *radii, int32_t n_cap,
                          int32_t nn_bins, double nn_max, int32_t per_replica, uint64_t *occ_hist,
                          uint64_t *occ_mom, uint64_t *nn_hist, double *points_out, int32_t *count_out,
                          double *nn_r2_out, int32_t *nn_idx_out, const char *what)
{
    // what can be refused without the batch comes first
    MMC_REQUIRE(n_probe >= 1 && n_probe <= (1 << 20), MMC_ERR_ARG, "%s: n_probe outside 1..2^20", what);
    MMC_REQUIRE(site >= -1 && site <= 2, MMC_ERR_ARG,
                "%s: site must be an atom slot 0..2 or -1 (the centre of mass)", what);
    MMC_REQUIRE(n_radii >= 1 && n_radii <= MMC_CAVITY_MAX_RADII, MMC_ERR_ARG, "%s: n_radii outside 1..%d", what,
                MMC_CAVITY_MAX_RADII);
    MMC_REQUIRE(radii, MMC_ERR_ARG, "%s: NULL radii", what);
    for (int k = 0; k < n_radii; k++)
        MMC_REQUIRE(std::isfinite(radii[k]) && radii[k] > 0.0 && (k == 0 || radii[k] > radii[k - 1]), MMC_ERR_ARG,
                    "%s: radii must be finite, > 0 and strictly ascending", what);
    MMC_REQUIRE(n_cap >= 1 && n_cap <= MMC_CAVITY_MAX_CAP, MMC_ERR_ARG, "%s: n_cap outside 1..%d", what,
                MMC_CAVITY_MAX_CAP);
    if (nn_hist) {
        MMC_REQUIRE(nn_bins >= 1 && nn_bins <= MMC_CAVITY_MAX_BINS, MMC_ERR_ARG, "%s: nn_bins outside 1..%d", what,
                    MMC_CAVITY_MAX_BINS);
        MMC_REQUIRE(std::isfinite(nn_max) && nn_max > 0.0, MMC_ERR_ARG, "%s: nn_max must be finite and > 0", what);
    }
    MMC_REQUIRE(occ_hist || occ_mom || nn_hist, MMC_ERR_ARG,
                "%s: give at least one of occ_hist, occ_mom and nn_hist", what);
    MMC_REQUIRE(!at || points_in, MMC_ERR_ARG, "%s: NULL points_in", what);
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    const int64_t R = s.R, N = s.n_mol, P = n_probe;
    if (at)
        for (int64_t q = 0; q < 3 * R * P; q++)
            MMC_REQUIRE(std::isfinite(points_in[q]), MMC_ERR_ARG, "%s: non-finite points_in", what);
    const double box_min = min_box(s);
    MMC_REQUIRE(radii[n_radii - 1] <= box_min / 2.0, MMC_ERR_ARG,
                "%s: radius %g exceeds half of the smallest box %g", what, radii[n_radii - 1], box_min);
    // the moment sums: a probe adds at most N^2
    MMC_REQUIRE((unsigned __int128)N * (unsigned __int128)N * (unsigned __int128)R * (unsigned __int128)P
                    < ((unsigned __int128)1 << 63),
                MMC_ERR_ARG, "%s: N^2 x replicas x n_probe reaches 2^63: the moment sums could wrap", what);
    STRUCT_STATE(b);
    BATCH_USABLE(b);
    MMC_REQUIRE(N >= 1 && N <= (1 << 21), MMC_ERR_UNSUPPORTED, "%s: 1 .. 2^21 molecules", what);
    // (a batch holds three-atom molecules only, mmc_batch_create: slots 0..2 exist in every molecule)

    // device scratch: the counters first (zeroed), then what is asked for per probe
    const int K = n_radii;
    const int64_t n_rep = per_replica ? R : 1;
    const size_t n_occ = occ_hist ? (size_t)K * (n_cap + 1) : 0, n_nn = nn_hist ? (size_t)nn_bins + 1 : 0;
    const size_t oh_bytes = 8 * (size_t)n_rep * n_occ, om_bytes = 16 * (size_t)n_rep * K,
                 nh_bytes = 8 * (size_t)n_rep * n_nn;
    const size_t pt_bytes = 24 * (size_t)(R * P), ct_bytes = 4 * (size_t)(R * P) * K, r2_bytes = 8 * (size_t)(R * P),
                 ix_bytes = 4 * (size_t)(R * P);
    ObsCall oc(b);
    const size_t o_oh = oc.take(oh_bytes), o_om = oc.take(occ_mom ? om_bytes : 0), o_nh = oc.take(nh_bytes),
                 o_pt = oc.take(at || points_out ? pt_bytes : 0), o_ct = oc.take(count_out ? ct_bytes : 0),
                 o_r2 = oc.take(nn_r2_out ? r2_bytes : 0), o_ix = oc.take(nn_idx_out ? ix_bytes : 0);
    MMC_TRY(oc.alloc());

    CavityArgs ca{};
    ca.box_r = s.pb.on ? s.pb.d_box : nullptr;
    ca.points_in = at ? oc.at<double>(o_pt) : nullptr;
    ca.points_out = (!at && points_out) ? oc.at<double>(o_pt) : nullptr;
    ca.occ_hist = occ_hist ? oc.at<unsigned long long>(o_oh) : nullptr;
    ca.occ_mom = occ_mom ? oc.at<unsigned long long>(o_om) : nullptr;
    ca.nn_hist = nn_hist ? oc.at<unsigned long long>(o_nh) : nullptr;
    ca.count = count_out ? oc.at<int32_t>(o_ct) : nullptr;
    ca.nn_r2 = nn_r2_out ? oc.at<double>(o_r2) : nullptr;
    ca.nn_idx = nn_idx_out ? oc.at<int32_t>(o_ix) : nullptr;
    for (int k = 0; k < CV_MAX_RADII; k++)
        ca.rad2[k] = k < K ? radii[k] * radii[k] : 0.0;
    ca.rmax2 = ca.rad2[K - 1];
    ca.dr = nn_hist ? nn_max / nn_bins : 1.0;
    ca.seed = seed;
    ca.draw0 = draw0;
    ca.n_probe = (int32_t)P;
    ca.n_radii = K;
    ca.n_cap = n_cap;
    ca.nn_bins = nn_hist ? nn_bins : 0;
    ca.site = site;
    ca.per_replica = per_replica ? 1 : 0;
    ca.R = (int32_t)R;

    // waves per workgroup: as many as keep their counters within half of the LDS; the site positions
    // are staged when they fit in the rest
    const size_t per_wave = 4 * (n_occ + n_nn);
    const int nw = tile_waves(NBR_LDS_BYTES / 2, per_wave);
    const size_t lds_w = ((size_t)nw * per_wave + 15) & ~(size_t)15;
    const bool stage = stage_fits(b, lds_w, N, NBR_LDS_BYTES);
    const size_t lds = lds_w + (stage ? 24 * (size_t)N : 0);
    const unsigned g = obs_grid(b, nw, R * ((P + 63) / 64)), t = (unsigned)nw * 64; // a block of 64 probes is a wave's unit

    oc.zero(o_pt);
    if (at)
        oc.to_device(oc.at<double>(o_pt), points_in, pt_bytes);
    nbr_launch(oc, [](auto rec, auto st) { return k_cavity_lane<decltype(rec)::value, decltype(st)::value>; }, stage, g, t, lds, lds,
               ca);
    oc.fetch(occ_hist, oc.at<char>(o_oh), oh_bytes);
    oc.fetch(occ_mom, oc.at<char>(o_om), om_bytes);
    oc.fetch(nn_hist, oc.at<char>(o_nh), nh_bytes);
    oc.fetch(at ? nullptr : points_out, oc.at<char>(o_pt), pt_bytes);
    oc.fetch(count_out, oc.at<char>(o_ct), ct_bytes);
    oc.fetch(nn_r2_out, oc.at<char>(o_r2), r2_bytes);
    oc.fetch(nn_idx_out, oc.at<char>(o_ix), ix_bytes);
    return oc.finish(what);
}

extern "C" int32_t mmc_batch_cavity(mmc_batch *b, int64_t n_probe, uint64_t seed, int64_t draw0, int32_t site,
                                    int32_t n_radii, const double *radii, int32_t n_cap, int32_t nn_bins,
                                    double nn_max, int32_t per_replica, uint64_t *occ_hist, uint64_t *occ_mom,
                                    uint64_t *nn_hist, double *points_out, int32_t *count_out, double *nn_r2_out,
                                    int32_t *nn_idx_out)
{
    return cavity_run(b, n_probe, seed, draw0, nullptr, false, site, n_radii, radii, n_cap, nn_bins, nn_max,
                      per_replica, occ_hist, occ_mom, nn_hist, points_out, count_out, nn_r2_out, nn_idx_out,
                      "mmc_batch_cavity");
}

extern "C" int32_t mmc_batch_cavity_at(mmc_batch *b, int64_t n_probe, const double *points_in, int32_t site,
                                       int32_t n_radii, const double *radii, int32_t n_cap, int32_t nn_bins,
                                       double nn_max, int32_t per_replica, uint64_t *occ_hist, uint64_t *occ_mom,
                                       uint64_t *nn_hist, int32_t *count_out, double *nn_r2_out, int32_t *nn_idx_out)
{
    return cavity_run(b, n_probe, 0, 0, points_in, true, site, n_radii, radii, n_cap, nn_bins, nn_max, per_replica,
                      occ_hist, occ_mom, nn_hist, nullptr, count_out, nn_r2_out, nn_idx_out, "mmc_batch_cavity_at");
}
