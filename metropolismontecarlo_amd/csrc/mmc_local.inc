// mmc_local.inc -- host side of mmc_batch_local_order (include/mmc_hip.h, "Local order"; the
// kernels are in mmc_local.hpp).  Included by mmc_hip.hip after mmc_units.inc (ObsCall).
#include "mmc_local.hpp"

extern "C" int32_t mmc_batch_local_order(mmc_batch *b, double r_hb, double cos_hb, int32_t q_bins,
                                         int32_t per_replica, uint64_t *hb_hist, uint64_t *q_hist,
                                         double *q_sum, int32_t *nbr_out, double *q_out, uint8_t *hb_out)
{
    // what can be refused without the batch comes first
    MMC_REQUIRE(std::isfinite(r_hb) && r_hb > 0.0, MMC_ERR_ARG,
                "mmc_batch_local_order: r_hb must be finite and > 0");
    MMC_REQUIRE(cos_hb > 0.0 && cos_hb <= 1.0, MMC_ERR_ARG, "mmc_batch_local_order: cos_hb outside (0, 1]");
    MMC_REQUIRE(q_bins >= 1 && q_bins <= MMC_LOCAL_MAX_BINS, MMC_ERR_ARG,
                "mmc_batch_local_order: q_bins outside 1..%d", MMC_LOCAL_MAX_BINS);
    MMC_REQUIRE(hb_hist || q_hist || q_sum, MMC_ERR_ARG,
                "mmc_batch_local_order: give at least one of hb_hist, q_hist and q_sum");
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    const int64_t R = s.R, N = s.n_mol;
    const double box_min = min_box(s);
    MMC_REQUIRE(r_hb <= box_min / 2.0, MMC_ERR_ARG,
                "mmc_batch_local_order: r_hb %g exceeds half of the smallest box %g", r_hb, box_min);
    STRUCT_STATE(b);
    BATCH_USABLE(b);
    MMC_REQUIRE(N >= 5 && N <= (1 << 21), MMC_ERR_UNSUPPORTED,
                "mmc_batch_local_order: 5 .. 2^21 molecules (four neighbours of every molecule)");
    // (a batch holds three-atom molecules only, mmc_batch_create: slots 0..2 exist in every molecule)

    // device scratch: the counters first (zeroed), then what is asked for per molecule
    const int64_t n_rep = per_replica ? R : 1;
    const bool want_q = q_sum || q_out;
    const size_t hb_bytes = 8 * (size_t)n_rep * LO_HB_ROWS, qh_bytes = 8 * (size_t)n_rep * q_bins;
    const size_t qs_bytes = 16 * (size_t)R, qa_bytes = 8 * (size_t)(R * N), nb_bytes = 16 * (size_t)(R * N),
                 hm_bytes = 2 * (size_t)(R * N);
    ObsCall oc(b);
    const size_t o_hb = oc.take(hb_bytes), o_qh = oc.take(qh_bytes), o_qs = oc.take(q_sum ? qs_bytes : 0),
                 o_qa = oc.take(want_q ? qa_bytes : 0), o_nb = oc.take(nbr_out ? nb_bytes : 0),
                 o_hm = oc.take(hb_out ? hm_bytes : 0);
    MMC_TRY(oc.alloc());

    LocalArgs la{};
    la.box_r = s.pb.on ? s.pb.d_box : nullptr;
    la.hb_hist = oc.at<unsigned long long>(o_hb);
    la.q_hist = oc.at<unsigned long long>(o_qh);
    la.q_all = want_q ? oc.at<double>(o_qa) : nullptr;
    la.nbr = nbr_out ? oc.at<int32_t>(o_nb) : nullptr;
    la.hb = hb_out ? oc.at<uint8_t>(o_hm) : nullptr;
    la.rhb2 = r_hb * r_hb;
    la.cos2 = cos_hb * cos_hb;
    la.q_scale = q_bins / 4.0;
    la.q_bins = q_bins;
    la.per_replica = per_replica ? 1 : 0;
    la.R = (int32_t)R;

    // waves per workgroup: as many as keep their counters and candidate lists within half of the LDS;
    // the O positions are staged when they fit in the rest
    const size_t per_wave = 4 * ((size_t)q_bins + LO_HB_ROWS + NBR_CAND);
    const int nw = tile_waves(NBR_LDS_BYTES / 2, per_wave);
    const size_t lds_w = ((size_t)nw * per_wave + 15) & ~(size_t)15;
    const bool stage = stage_fits(b, lds_w, N, NBR_LDS_BYTES);
    const size_t lds = lds_w + (stage ? 24 * (size_t)N : 0);
    const unsigned g = obs_grid(b, nw, R * N), t = (unsigned)nw * 64; // a molecule is a wave's unit

    oc.zero(o_qs);
    nbr_launch(oc, [](auto rec, auto st) { return k_local_order_wave<decltype(rec)::value, decltype(st)::value>; }, stage, g, t,
               lds, lds, la);
    if (oc.e == hipSuccess && q_sum)
        k_local_qsum<<<(unsigned)((R + NBR_WAVES - 1) / NBR_WAVES), NBR_WAVES * 64, 0, oc.st>>>(
            la.q_all, oc.at<double>(o_qs), (int)N, (int)R);
    oc.launched();
    oc.fetch(hb_hist, oc.at<char>(o_hb), hb_bytes);
    oc.fetch(q_hist, oc.at<char>(o_qh), qh_bytes);
    oc.fetch(q_sum, oc.at<char>(o_qs), qs_bytes);
    oc.fetch(q_out, oc.at<char>(o_qa), qa_bytes);
    oc.fetch(nbr_out, oc.at<char>(o_nb), nb_bytes);
    oc.fetch(hb_out, oc.at<char>(o_hm), hm_bytes);
    return oc.finish("mmc_batch_local_order");
}
