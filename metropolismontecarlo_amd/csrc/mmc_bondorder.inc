// mmc_bondorder.inc -- host side of mmc_batch_bond_order (include/mmc_hip.h, "Bond order"; the
// kernels are in mmc_bondorder.hpp).  Included by mmc_hip.hip after mmc_shell.inc.
#include "mmc_bondorder.hpp"

static_assert(MMC_BO_MAX_NB == 16 && MMC_BO_MAX_NB <= BO_REC, "one lane per neighbour and per record slot");
static_assert(8 * (size_t)MMC_BO_MAX_MOL + 16 <= NBR_LDS_BYTES, "labels and sizes of a replica in one workgroup's LDS");
static_assert(MMC_BO_STATS == 8, "four counters of phase A, four of phase C");

#define BO_SCRATCH_BYTES ((size_t)256 << 20) // the chunk's records: see DESIGN.md, "Bond order"

extern "C" int32_t mmc_batch_bond_order(mmc_batch *b, int32_t l, double r_nb, int32_t n_nb, double a_lo, double a_hi,
                                        double b_lo, double b_hi, int32_t min_a, int32_t min_ab, int32_t q_bins,
                                        int32_t c_bins, int32_t per_replica, uint64_t *q_hist, uint64_t *qbar_hist,
                                        uint64_t *c_hist, uint64_t *ab_hist, uint64_t *size_hist, int64_t *stats,
                                        double *sums, double *q_out, double *qbar_out, int32_t *nbr_out, uint8_t *ab_out,
                                        int32_t *label_out)
{
    // what can be refused without the batch comes first
    MMC_REQUIRE(l == 3 || l == 4 || l == 6, MMC_ERR_ARG, "mmc_batch_bond_order: l must be 3, 4 or 6");
    MMC_REQUIRE(std::isfinite(r_nb) && r_nb > 0.0, MMC_ERR_ARG, "mmc_batch_bond_order: r_nb must be finite and > 0");
    MMC_REQUIRE(n_nb >= 1 && n_nb <= MMC_BO_MAX_NB, MMC_ERR_ARG, "mmc_batch_bond_order: n_nb outside 1..%d",
                MMC_BO_MAX_NB);
    MMC_REQUIRE(q_bins >= 1 && q_bins <= MMC_BO_MAX_BINS, MMC_ERR_ARG, "mmc_batch_bond_order: q_bins outside 1..%d",
                MMC_BO_MAX_BINS);
    MMC_REQUIRE(c_bins >= 1 && c_bins <= MMC_BO_MAX_BINS, MMC_ERR_ARG, "mmc_batch_bond_order: c_bins outside 1..%d",
                MMC_BO_MAX_BINS);
    MMC_REQUIRE(!std::isnan(a_lo) && !std::isnan(a_hi), MMC_ERR_ARG, "mmc_batch_bond_order: a_lo or a_hi is NaN");
    MMC_REQUIRE(!std::isnan(b_lo) && !std::isnan(b_hi), MMC_ERR_ARG, "mmc_batch_bond_order: b_lo or b_hi is NaN");
    MMC_REQUIRE(q_hist || qbar_hist || c_hist || ab_hist || size_hist || stats || sums || q_out || qbar_out || nbr_out ||
                    ab_out || label_out,
                MMC_ERR_ARG, "mmc_batch_bond_order: give at least one output");
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    const int64_t R = s.R, N = s.n_mol;
    const double box_min = min_box(s);
    MMC_REQUIRE(r_nb <= box_min / 2.0, MMC_ERR_ARG, "mmc_batch_bond_order: r_nb %g exceeds half of the smallest box %g",
                r_nb, box_min);
    STRUCT_STATE(b);
    BATCH_USABLE(b);
    MMC_REQUIRE(N >= 2 && N <= MMC_BO_MAX_MOL, MMC_ERR_UNSUPPORTED,
                "mmc_batch_bond_order: N = %lld molecules: 2 .. %d (the cluster labels of a replica stay in LDS)",
                (long long)N, MMC_BO_MAX_MOL);

    // the phases that the outputs need
    const bool phase_c = size_hist || stats || label_out;
    const bool phase_b = phase_c || qbar_hist || c_hist || ab_hist || sums || qbar_out || ab_out;
    const bool want_q = sums || q_out, want_qbar = sums || qbar_out;

    // replicas per chunk: what the records of a chunk (and its q_l, qbar_l where only the sums want
    // them) leave of the budget
    const size_t per_mol = 8 * BO_REC + 4 * MMC_BO_MAX_NB + 4 + 1 + (want_q && !q_out ? 8 : 0) + (want_qbar && !qbar_out ? 8 : 0);
    int64_t chunk = b->bond_chunk > 0 ? b->bond_chunk : (int64_t)(BO_SCRATCH_BYTES / (per_mol * (size_t)N));
    chunk = std::max<int64_t>(1, std::min(chunk, R));
    const int64_t CN = chunk * N;

    // device scratch: the counters first (zeroed), then the outputs per molecule, then the chunk's
    const int64_t n_rep = per_replica ? R : 1;
    const size_t st_bytes = 8 * (size_t)MMC_BO_STATS * (size_t)R, qh_bytes = 8 * (size_t)n_rep * ((size_t)q_bins + 1),
                 ch_bytes = 8 * (size_t)n_rep * ((size_t)c_bins + 1), ab_bytes = 8 * (size_t)n_rep * 289,
                 sz_bytes = 8 * (size_t)n_rep * ((size_t)N + 1), sm_bytes = 16 * (size_t)R;
    const size_t pm_bytes = 8 * (size_t)(R * N), nb_bytes = 4 * (size_t)MMC_BO_MAX_NB * (size_t)(R * N),
                 a2_bytes = 2 * (size_t)(R * N), lb_bytes = 4 * (size_t)(R * N);
    ObsCall oc(b);
    const size_t o_st = oc.take(st_bytes), o_qh = oc.take(q_hist ? qh_bytes : 0), o_bh = oc.take(qbar_hist ? qh_bytes : 0),
                 o_ch = oc.take(c_hist ? ch_bytes : 0), o_ab = oc.take(ab_hist ? ab_bytes : 0),
                 o_sz = oc.take(size_hist ? sz_bytes : 0), o_s1 = oc.take(sums ? sm_bytes : 0),
                 o_s2 = oc.take(sums ? sm_bytes : 0);
    const size_t o_zero_end = oc.end;
    const size_t o_qa = oc.take(want_q ? (q_out ? pm_bytes : 8 * (size_t)CN) : 0),
                 o_ba = oc.take(want_qbar ? (qbar_out ? pm_bytes : 8 * (size_t)CN) : 0),
                 o_nb = oc.take(nbr_out ? nb_bytes : 0), o_a2 = oc.take(ab_out ? a2_bytes : 0),
                 o_lb = oc.take(label_out ? lb_bytes : 0), o_nm = oc.take(8 * 7), o_rec = oc.take(8 * BO_REC * (size_t)CN),
                 o_cn = oc.take(4 * MMC_BO_MAX_NB * (size_t)CN), o_cs = oc.take(4 * (size_t)CN), o_so = oc.take((size_t)CN);
    MMC_TRY(oc.alloc());

    // the constants of the header
    const double PI = 3.141592653589793;
    double norm[7] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    for (int m = 0; m <= l; m++) {
        double F = 1.0;
        for (int k = l - m + 1; k <= l + m; k++)
            F = F * (double)k;
        norm[m] = std::sqrt(((double)(2 * l + 1) / (4.0 * PI)) / F);
    }

    BondArgs ba{};
    ba.box_r = s.pb.on ? s.pb.d_box : nullptr;
    ba.norm = oc.at<double>(o_nm);
    ba.rec = oc.at<double>(o_rec);
    ba.nb = oc.at<int32_t>(o_cn);
    ba.st = oc.at<int32_t>(o_cs);
    ba.solid = oc.at<uint8_t>(o_so);
    ba.stats = stats ? oc.at<unsigned long long>(o_st) : nullptr;
    ba.q_hist = q_hist ? oc.at<unsigned long long>(o_qh) : nullptr;
    ba.qbar_hist = qbar_hist ? oc.at<unsigned long long>(o_bh) : nullptr;
    ba.c_hist = c_hist ? oc.at<unsigned long long>(o_ch) : nullptr;
    ba.ab_hist = ab_hist ? oc.at<unsigned long long>(o_ab) : nullptr;
    ba.size_hist = size_hist ? oc.at<unsigned long long>(o_sz) : nullptr;
    ba.nbr_out = nbr_out ? oc.at<int32_t>(o_nb) : nullptr;
    ba.label_out = label_out ? oc.at<int32_t>(o_lb) : nullptr;
    ba.ab_out = ab_out ? oc.at<uint8_t>(o_a2) : nullptr;
    ba.q_all = want_q ? oc.at<double>(o_qa) : nullptr;
    ba.qbar_all = want_qbar ? oc.at<double>(o_ba) : nullptr;
    ba.rnb2 = r_nb * r_nb;
    ba.K = (4.0 * PI) / (double)(2 * l + 1);
    ba.a_lo = a_lo;
    ba.a_hi = a_hi;
    ba.b_lo = b_lo;
    ba.b_hi = b_hi;
    ba.q_scale = (double)q_bins;
    ba.c_scale = c_bins / 2.0;
    ba.l = l;
    ba.n_nb = n_nb;
    ba.min_a = min_a;
    ba.min_ab = min_ab;
    ba.q_bins = q_bins;
    ba.c_bins = c_bins;
    ba.per_replica = per_replica ? 1 : 0;

    // phase A: four waves, their lists and blocks beside the counters; the O positions where they fit
    const int nw = NBR_WAVES;
    const size_t hs_a = 4 + (q_hist ? (size_t)q_bins + 1 : 0);
    const size_t lds_w = ((size_t)nw * (NBR_LIST_BYTES + BO_Y_BYTES) + 4 * hs_a + 15) & ~(size_t)15;
    const bool stage = stage_fits(b, lds_w, N, NBR_LDS_BYTES);
    const size_t lds_a = lds_w + (stage ? 24 * (size_t)N : 0);
    const size_t lds_b = 4 * ((qbar_hist ? (size_t)q_bins + 1 : 0) + (c_hist ? (size_t)c_bins + 1 : 0) + (ab_hist ? 289 : 0));
    const size_t lds_c = 8 * (size_t)N + 16;
    const unsigned t = (unsigned)nw * 64;

    oc.zero(o_zero_end); // every counter
    oc.to_device(oc.at<double>(o_nm), norm, sizeof norm); // (norm outlives the copy: finish() drains the stream)
    for (int64_t r0 = 0; r0 < R; r0 += chunk) {
        const int64_t nr = std::min(chunk, R - r0);
        ba.r0 = (int32_t)r0;
        ba.nr = (int32_t)nr;
        const unsigned g = obs_grid(b, nw, nr * N); // a molecule is a wave's unit
        ba.q_r0 = q_out ? 0 : (int32_t)r0;
        nbr_launch(oc, [](auto rec, auto st) { return k_bond_qlm<decltype(rec)::value, decltype(st)::value>; }, stage, g, t, lds_a,
                   lds_a, ba);
        const unsigned gq = (unsigned)((nr + NBR_WAVES - 1) / NBR_WAVES);
        if (oc.e == hipSuccess && sums)
            k_local_qsum<<<gq, NBR_WAVES * 64, 0, oc.st>>>(ba.q_all + (q_out ? r0 * N : 0), oc.at<double>(o_s1) + 2 * r0, (int)N,
                                                          (int)nr);
        oc.launched();
        if (oc.e == hipSuccess && phase_b) {
            ba.q_r0 = qbar_out ? 0 : (int32_t)r0;
            k_bond_corr<<<g, t, lds_b, oc.st>>>(ba, (int)N);
        }
        oc.launched();
        if (oc.e == hipSuccess && sums)
            k_local_qsum<<<gq, NBR_WAVES * 64, 0, oc.st>>>(ba.qbar_all + (qbar_out ? r0 * N : 0), oc.at<double>(o_s2) + 2 * r0,
                                                          (int)N, (int)nr);
        oc.launched();
        if (oc.e == hipSuccess && phase_c)
            k_bond_clusters<<<(unsigned)nr, BO_C_THREADS, lds_c, oc.st>>>(ba, (int)N);
        oc.launched();
    }
    oc.fetch(q_hist, oc.at<char>(o_qh), qh_bytes);
    oc.fetch(qbar_hist, oc.at<char>(o_bh), qh_bytes);
    oc.fetch(c_hist, oc.at<char>(o_ch), ch_bytes);
    oc.fetch(ab_hist, oc.at<char>(o_ab), ab_bytes);
    oc.fetch(size_hist, oc.at<char>(o_sz), sz_bytes);
    oc.fetch(stats, oc.at<char>(o_st), st_bytes);
    oc.fetch(q_out, oc.at<char>(o_qa), pm_bytes);
    oc.fetch(qbar_out, oc.at<char>(o_ba), pm_bytes);
    oc.fetch(nbr_out, oc.at<char>(o_nb), nb_bytes);
    oc.fetch(ab_out, oc.at<char>(o_a2), a2_bytes);
    oc.fetch(label_out, oc.at<char>(o_lb), lb_bytes);
    const double *h1 = sums ? reinterpret_cast<const double *>(oc.stage(oc.at<char>(o_s1), sm_bytes)) : nullptr;
    const double *h2 = sums ? reinterpret_cast<const double *>(oc.stage(oc.at<char>(o_s2), sm_bytes)) : nullptr;
    MMC_TRY(oc.finish("mmc_batch_bond_order"));
    if (sums) // (sum q_l, defined, sum qbar_l, defined) per replica
        for (int64_t r = 0; r < R; r++) {
            sums[4 * r] = h1[2 * r];
            sums[4 * r + 1] = h1[2 * r + 1];
            sums[4 * r + 2] = h2[2 * r];
            sums[4 * r + 3] = h2[2 * r + 1];
        }
    return MMC_OK;
}
