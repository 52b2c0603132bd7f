// mmc_local.inc -- host side of mmc_batch_local_order (include/mmc_hip.h, "Local order"; the
// kernels are in mmc_local.hpp).  Included by mmc_hip.hip after mmc_struct.inc, whose state checks
// it shares, and after mmc_units.inc, whose device scratch (obs_scratch) it uses.
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
    const double min_box = s.pb.on ? *std::min_element(s.pb.box.begin(), s.pb.box.end()) : s.bv.box;
    MMC_REQUIRE(r_hb <= min_box / 2.0, MMC_ERR_ARG,
                "mmc_batch_local_order: r_hb %g exceeds half of the smallest box %g", r_hb, min_box);
    STRUCT_STATE(b);
    BATCH_USABLE(b);
    MMC_REQUIRE(N >= 5 && N <= (1 << 21), MMC_ERR_UNSUPPORTED,
                "mmc_batch_local_order: 5 .. 2^21 molecules (four neighbours of every molecule)");
    // (a batch holds three-atom molecules only, mmc_batch_create: slots 0..2 exist in every molecule)

    // device scratch: the counters first (zeroed), then what is asked for per molecule
    const int64_t n_rep = per_replica ? R : 1;
    const bool want_q = q_sum || q_out;
    auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t hb_bytes = up16(8 * (size_t)n_rep * LO_HB_ROWS), qh_bytes = up16(8 * (size_t)n_rep * q_bins);
    const size_t qs_bytes = up16(q_sum ? 16 * (size_t)R : 0), qa_bytes = up16(want_q ? 8 * (size_t)(R * N) : 0);
    const size_t nb_bytes = up16(nbr_out ? 16 * (size_t)(R * N) : 0), hm_bytes = up16(hb_out ? 2 * (size_t)(R * N) : 0);
    char *d_buf = nullptr;
    MMC_TRY(obs_scratch(b, hb_bytes + qh_bytes + qs_bytes + qa_bytes + nb_bytes + hm_bytes, &d_buf));
    char *d_hb = d_buf, *d_qh = d_hb + hb_bytes, *d_qs = d_qh + qh_bytes, *d_qa = d_qs + qs_bytes,
         *d_nb = d_qa + qa_bytes, *d_hm = d_nb + nb_bytes;

    LocalArgs la{};
    la.box_r = s.pb.on ? s.pb.d_box : nullptr;
    la.hb_hist = reinterpret_cast<unsigned long long *>(d_hb);
    la.q_hist = reinterpret_cast<unsigned long long *>(d_qh);
    la.q_all = want_q ? reinterpret_cast<double *>(d_qa) : nullptr;
    la.nbr = nbr_out ? reinterpret_cast<int32_t *>(d_nb) : nullptr;
    la.hb = hb_out ? reinterpret_cast<uint8_t *>(d_hm) : nullptr;
    la.rhb2 = r_hb * r_hb;
    la.cos2 = cos_hb * cos_hb;
    la.q_scale = q_bins / 4.0;
    la.q_bins = q_bins;
    la.per_replica = per_replica ? 1 : 0;
    la.R = (int32_t)R;

    // waves per workgroup: as many of LO_WAVES as keep their counters and candidate lists within half
    // of the LDS; the O positions are staged when they fit in the rest
    const size_t per_wave = 4 * ((size_t)q_bins + LO_HB_ROWS + LO_CAND);
    int nw = LO_WAVES;
    while (nw > 1 && (size_t)nw * per_wave > LO_LDS_BYTES / 2)
        nw >>= 1;
    const size_t lds_w = up16((size_t)nw * per_wave);
    const bool stage = b->local_stage && lds_w + 24 * (size_t)N <= LO_LDS_BYTES;
    const size_t lds = lds_w + (stage ? 24 * (size_t)N : 0);
    // persistent workgroups: four waves per SIMD of every compute unit, or option "wave_wgs"; no more
    // than give every wave a molecule
    int64_t wgs = b->wave_wgs > 0 ? b->wave_wgs : (int64_t)(16 / nw) * b->n_cus;
    wgs = std::max<int64_t>(1, std::min(wgs, (R * N + nw - 1) / nw));

    hipStream_t st = s.stream;
    hipError_t e = hipMemsetAsync(d_buf, 0, hb_bytes + qh_bytes, st);
    if (e == hipSuccess) {
        const bool use_rec = struct_use_rec(b);
        const unsigned g = (unsigned)wgs, t = (unsigned)nw * 64;
        if (use_rec && stage)
            k_local_order_wave<true, true><<<g, t, lds, st>>>(s.bv, s.rec, la);
        else if (use_rec)
            k_local_order_wave<true, false><<<g, t, lds, st>>>(s.bv, s.rec, la);
        else if (stage)
            k_local_order_wave<false, true><<<g, t, lds, st>>>(s.bv, nullptr, la);
        else
            k_local_order_wave<false, false><<<g, t, lds, st>>>(s.bv, nullptr, la);
        e = hipGetLastError();
    }
    if (e == hipSuccess && q_sum) {
        k_local_qsum<<<(unsigned)((R + LO_WAVES - 1) / LO_WAVES), LO_WAVES * 64, 0, st>>>(
            la.q_all, reinterpret_cast<double *>(d_qs), (int)N, (int)R);
        e = hipGetLastError();
    }
    // everything goes through host copies: the caller's arrays are written only on success
    const size_t out_bytes[6] = { hb_hist ? 8 * (size_t)n_rep * LO_HB_ROWS : 0, q_hist ? 8 * (size_t)n_rep * q_bins : 0,
                                  q_sum ? 16 * (size_t)R : 0, q_out ? 8 * (size_t)(R * N) : 0,
                                  nbr_out ? 16 * (size_t)(R * N) : 0, hb_out ? 2 * (size_t)(R * N) : 0 };
    const char *d_src[6] = { d_hb, d_qh, d_qs, d_qa, d_nb, d_hm };
    void *dst[6] = { hb_hist, q_hist, q_sum, q_out, nbr_out, hb_out };
    std::vector<char> h_out[6];
    for (int k = 0; k < 6 && e == hipSuccess; k++) {
        if (!out_bytes[k])
            continue;
        h_out[k].resize(out_bytes[k]);
        e = hipMemcpyAsync(h_out[k].data(), d_src[k], out_bytes[k], hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);
    else
        (void)hipStreamSynchronize(st); // (the host buffers of copies already queued outlive them)
    MMC_REQUIRE(e == hipSuccess, MMC_ERR_HIP, "mmc_batch_local_order failed: %s", hipGetErrorString(e));
    for (int k = 0; k < 6; k++)
        if (out_bytes[k])
            memcpy(dst[k], h_out[k].data(), out_bytes[k]);
    return MMC_OK;
}
