// mmc_shell.inc -- host side of mmc_batch_shell_order (include/mmc_hip.h, "Shell order"; the kernel
// is in mmc_shell.hpp).  Included by mmc_hip.hip after mmc_local.inc (k_local_qsum, tile_waves).
#include "mmc_shell.hpp"

static_assert(MMC_SHELL_CAP == 64, "one lane per listed neighbour");

extern "C" int32_t mmc_batch_shell_order(mmc_batch *b, double r_list, double r_lsi, double r_ang, double r_hb, double cos_hb,
                                         int32_t n_rank, int32_t r_bins, int32_t lsi_bins, double lsi_max, int32_t ang_bins,
                                         int32_t zeta_bins, double zeta_lo, double zeta_hi, int32_t per_replica,
                                         uint64_t *rank_hist, uint64_t *lsi_hist, uint64_t *ang_hist, uint64_t *zeta_hist,
                                         uint64_t *flagged, double *sums, int32_t *count_out, int32_t *nbr_out,
                                         double *lsi_out, double *zeta_out)
{
    // what can be refused without the batch comes first
    MMC_REQUIRE(std::isfinite(r_list) && r_list > 0.0, MMC_ERR_ARG,
                "mmc_batch_shell_order: r_list must be finite and > 0");
    MMC_REQUIRE(r_lsi > 0.0 && r_lsi <= r_list, MMC_ERR_ARG, "mmc_batch_shell_order: r_lsi outside (0, r_list]");
    MMC_REQUIRE(r_ang > 0.0 && r_ang <= r_list, MMC_ERR_ARG, "mmc_batch_shell_order: r_ang outside (0, r_list]");
    MMC_REQUIRE(r_hb > 0.0 && r_hb <= r_list, MMC_ERR_ARG, "mmc_batch_shell_order: r_hb outside (0, r_list]");
    MMC_REQUIRE(cos_hb > 0.0 && cos_hb <= 1.0, MMC_ERR_ARG, "mmc_batch_shell_order: cos_hb outside (0, 1]");
    MMC_REQUIRE(n_rank >= 1 && n_rank <= MMC_SHELL_MAX_RANK, MMC_ERR_ARG,
                "mmc_batch_shell_order: n_rank outside 1..%d", MMC_SHELL_MAX_RANK);
    MMC_REQUIRE(r_bins >= 1 && r_bins <= MMC_SHELL_MAX_BINS, MMC_ERR_ARG,
                "mmc_batch_shell_order: r_bins outside 1..%d", MMC_SHELL_MAX_BINS);
    MMC_REQUIRE(lsi_bins >= 1 && lsi_bins <= MMC_SHELL_MAX_BINS, MMC_ERR_ARG,
                "mmc_batch_shell_order: lsi_bins outside 1..%d", MMC_SHELL_MAX_BINS);
    MMC_REQUIRE(std::isfinite(lsi_max) && lsi_max > 0.0, MMC_ERR_ARG,
                "mmc_batch_shell_order: lsi_max must be finite and > 0");
    MMC_REQUIRE(ang_bins >= 1 && ang_bins <= MMC_SHELL_MAX_BINS, MMC_ERR_ARG,
                "mmc_batch_shell_order: ang_bins outside 1..%d", MMC_SHELL_MAX_BINS);
    MMC_REQUIRE(zeta_bins >= 1 && zeta_bins <= MMC_SHELL_MAX_BINS, MMC_ERR_ARG,
                "mmc_batch_shell_order: zeta_bins outside 1..%d", MMC_SHELL_MAX_BINS);
    MMC_REQUIRE(std::isfinite(zeta_lo) && std::isfinite(zeta_hi) && zeta_lo < zeta_hi, MMC_ERR_ARG,
                "mmc_batch_shell_order: zeta_lo < zeta_hi, both finite");
    MMC_REQUIRE(rank_hist || lsi_hist || ang_hist || zeta_hist || sums, MMC_ERR_ARG,
                "mmc_batch_shell_order: give at least one of rank_hist, lsi_hist, ang_hist, zeta_hist and sums");
    // a workgroup's counters: flagged, then the histograms that are asked for; they and one wave's
    // list must fit in the half of the LDS that the positions leave
    const size_t w_rank = rank_hist ? (size_t)n_rank * ((size_t)r_bins + 1) : 0, w_lsi = lsi_hist ? (size_t)lsi_bins + 1 : 0,
                 w_ang = ang_hist ? (size_t)ang_bins + 1 : 0, w_zeta = zeta_hist ? (size_t)zeta_bins + 1 : 0;
    const size_t hs = 1 + w_rank + w_lsi + w_ang + w_zeta;
    MMC_REQUIRE(hs <= MMC_SHELL_MAX_WORDS, MMC_ERR_ARG,
                "mmc_batch_shell_order: the bins of the histograms asked for (n_rank (r_bins + 1) + (lsi_bins + 1) + "
                "(ang_bins + 1) + (zeta_bins + 1) = %zu) exceed %d",
                hs - 1, MMC_SHELL_MAX_WORDS - 1);
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    const int64_t R = s.R, N = s.n_mol;
    const double box_min = min_box(s);
    MMC_REQUIRE(r_list <= box_min / 2.0, MMC_ERR_ARG,
                "mmc_batch_shell_order: r_list %g exceeds half of the smallest box %g", r_list, box_min);
    STRUCT_STATE(b);
    BATCH_USABLE(b);
    MMC_REQUIRE(N >= 2 && N <= (1 << 21), MMC_ERR_UNSUPPORTED, "mmc_batch_shell_order: 2 .. 2^21 molecules");
    // (a batch holds three-atom molecules only, mmc_batch_create: slots 0..2 exist in every molecule)

    // device scratch: the counters first (zeroed), then what is asked for per molecule
    const int64_t n_rep = per_replica ? R : 1;
    const bool want_lsi = sums || lsi_out, want_zeta = sums || zeta_out;
    const size_t fl_bytes = 8 * (size_t)R, rk_bytes = 8 * (size_t)n_rep * w_rank, ls_bytes = 8 * (size_t)n_rep * w_lsi,
                 an_bytes = 8 * (size_t)n_rep * w_ang, ze_bytes = 8 * (size_t)n_rep * w_zeta;
    const size_t sm_bytes = 16 * (size_t)R, pm_bytes = 8 * (size_t)(R * N), ct_bytes = 4 * (size_t)(R * N),
                 nb_bytes = 4 * (size_t)MMC_SHELL_NBR * (size_t)(R * N);
    ObsCall oc(b);
    const size_t o_fl = oc.take(fl_bytes), o_rk = oc.take(rk_bytes), o_ls = oc.take(ls_bytes), o_an = oc.take(an_bytes),
                 o_ze = oc.take(ze_bytes), o_s1 = oc.take(sums ? sm_bytes : 0), o_s2 = oc.take(sums ? sm_bytes : 0),
                 o_la = oc.take(want_lsi ? pm_bytes : 0), o_za = oc.take(want_zeta ? pm_bytes : 0),
                 o_ct = oc.take(count_out ? ct_bytes : 0), o_nb = oc.take(nbr_out ? nb_bytes : 0);
    MMC_TRY(oc.alloc());

    ShellArgs sa{};
    sa.box_r = s.pb.on ? s.pb.d_box : nullptr;
    sa.flagged = oc.at<unsigned long long>(o_fl);
    sa.rank_hist = rank_hist ? oc.at<unsigned long long>(o_rk) : nullptr;
    sa.lsi_hist = lsi_hist ? oc.at<unsigned long long>(o_ls) : nullptr;
    sa.ang_hist = ang_hist ? oc.at<unsigned long long>(o_an) : nullptr;
    sa.zeta_hist = zeta_hist ? oc.at<unsigned long long>(o_ze) : nullptr;
    sa.count = count_out ? oc.at<int32_t>(o_ct) : nullptr;
    sa.nbr = nbr_out ? oc.at<int32_t>(o_nb) : nullptr;
    sa.lsi_all = want_lsi ? oc.at<double>(o_la) : nullptr;
    sa.zeta_all = want_zeta ? oc.at<double>(o_za) : nullptr;
    sa.rl2 = r_list * r_list;
    sa.rlsi2 = r_lsi * r_lsi;
    sa.rang2 = r_ang * r_ang;
    sa.rhb2 = r_hb * r_hb;
    sa.cos2 = cos_hb * cos_hb;
    sa.inv_dr = r_bins / r_list;
    sa.lsi_scale = lsi_bins / lsi_max;
    sa.ang_scale = ang_bins / 2.0;
    sa.zeta_lo = zeta_lo;
    sa.zeta_scale = zeta_bins / (zeta_hi - zeta_lo);
    sa.n_rank = n_rank;
    sa.r_bins = r_bins;
    sa.lsi_bins = lsi_bins;
    sa.ang_bins = ang_bins;
    sa.zeta_bins = zeta_bins;
    sa.o_lsi = (int32_t)(1 + w_rank);
    sa.o_ang = (int32_t)(sa.o_lsi + w_lsi);
    sa.o_zeta = (int32_t)(sa.o_ang + w_ang);
    sa.hs = (int32_t)hs;
    sa.per_replica = per_replica ? 1 : 0;
    sa.R = (int32_t)R;

    // waves per workgroup: as many as keep their lists beside the counters within half of the LDS; the
    // O positions are staged when they fit in the rest
    const int nw = tile_waves(NBR_LDS_BYTES / 2 + 4 * hs, NBR_LIST_BYTES);
    const size_t lds_w = ((size_t)nw * NBR_LIST_BYTES + 4 * hs + 15) & ~(size_t)15;
    const bool stage = stage_fits(b, lds_w, N, NBR_LDS_BYTES);
    const size_t lds = lds_w + (stage ? 24 * (size_t)N : 0);
    const unsigned g = obs_grid(b, nw, R * N), t = (unsigned)nw * 64; // a molecule is a wave's unit

    oc.zero(o_s1); // every counter
    nbr_launch(oc, [](auto rec, auto st) { return k_shell_order_wave<decltype(rec)::value, decltype(st)::value>; }, stage, g, t,
               lds, lds, sa);
    const unsigned gq = (unsigned)((R + NBR_WAVES - 1) / NBR_WAVES);
    if (oc.e == hipSuccess && sums) {
        k_local_qsum<<<gq, NBR_WAVES * 64, 0, oc.st>>>(sa.lsi_all, oc.at<double>(o_s1), (int)N, (int)R);
        k_local_qsum<<<gq, NBR_WAVES * 64, 0, oc.st>>>(sa.zeta_all, oc.at<double>(o_s2), (int)N, (int)R);
    }
    oc.launched();
    oc.fetch(flagged, oc.at<char>(o_fl), fl_bytes);
    oc.fetch(rank_hist, oc.at<char>(o_rk), rk_bytes);
    oc.fetch(lsi_hist, oc.at<char>(o_ls), ls_bytes);
    oc.fetch(ang_hist, oc.at<char>(o_an), an_bytes);
    oc.fetch(zeta_hist, oc.at<char>(o_ze), ze_bytes);
    oc.fetch(count_out, oc.at<char>(o_ct), ct_bytes);
    oc.fetch(nbr_out, oc.at<char>(o_nb), nb_bytes);
    oc.fetch(lsi_out, oc.at<char>(o_la), pm_bytes);
    oc.fetch(zeta_out, oc.at<char>(o_za), pm_bytes);
    const double *h1 = sums ? reinterpret_cast<const double *>(oc.stage(oc.at<char>(o_s1), sm_bytes)) : nullptr;
    const double *h2 = sums ? reinterpret_cast<const double *>(oc.stage(oc.at<char>(o_s2), sm_bytes)) : nullptr;
    MMC_TRY(oc.finish("mmc_batch_shell_order"));
    if (sums) // (sum I, defined, sum zeta, defined) per replica
        for (int64_t r = 0; r < R; r++) {
            sums[4 * r] = h1[2 * r];
            sums[4 * r + 1] = h1[2 * r + 1];
            sums[4 * r + 2] = h2[2 * r];
            sums[4 * r + 3] = h2[2 * r + 1];
        }
    return MMC_OK;
}
