// mmc_orient.inc -- host side of mmc_batch_orient_corr (include/mmc_hip.h, "Orientational pair
// correlations"; the kernel is in mmc_orient.hpp).  Included by mmc_hip.hip after mmc_struct.inc,
// whose thresholds (rdf_thresholds) and state checks it shares, and after mmc_units.inc, whose
// device scratch (obs_scratch) it uses.
#include "mmc_orient.hpp"

extern "C" int32_t mmc_batch_orient_corr(mmc_batch *b, int32_t numbins, double r_max, int32_t per_replica,
                                         int64_t *hist)
{
    // what can be refused without the batch comes first
    MMC_REQUIRE(hist, MMC_ERR_ARG, "mmc_batch_orient_corr: NULL out pointer");
    MMC_REQUIRE(numbins >= 1 && numbins <= MMC_ORIENT_MAX_BINS, MMC_ERR_ARG,
                "mmc_batch_orient_corr: numbins outside 1..%d", MMC_ORIENT_MAX_BINS);
    MMC_REQUIRE(std::isfinite(r_max), MMC_ERR_ARG, "mmc_batch_orient_corr: r_max is not finite");
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    const int64_t R = s.R;
    double min_box = s.bv.box;
    if (s.pb.on) {
        MMC_REQUIRE(r_max > 0.0, MMC_ERR_ARG,
                    "mmc_batch_orient_corr: per-replica boxes have no common L/2: give r_max > 0");
        min_box = *std::min_element(s.pb.box.begin(), s.pb.box.end());
    }
    MMC_REQUIRE(!(r_max > 0.0) || r_max <= min_box / 2.0, MMC_ERR_ARG,
                "mmc_batch_orient_corr: r_max %g exceeds half of the smallest box %g", r_max, min_box);
    STRUCT_STATE(b);
    MMC_REQUIRE(s.n_mol >= 1 && s.n_mol <= (1 << 21), MMC_ERR_UNSUPPORTED,
                "mmc_batch_orient_corr: 1 .. 2^21 molecules (the tiles of a replica are counted in 32 bits)");
    // (a batch holds three-atom molecules only, mmc_batch_create: slots 0..2 exist in every molecule)

    // the bins of mmc_batch_rdf_sites: dr = side / 2 / numbins (gr.jl:5), else the caller's range
    const double dr = r_max > 0.0 ? r_max / numbins : (min_box / 2.0) / numbins;
    std::vector<double> thr;
    rdf_thresholds(dr, numbins, thr);

    const size_t rs = (size_t)numbins + 2;
    const size_t n_out = (size_t)(per_replica ? R : 1) * 4 * rs;
    const size_t hist_bytes = sizeof(unsigned long long) * n_out, thr_bytes = sizeof(double) * thr.size();
    char *d_buf = nullptr;
    MMC_TRY(obs_scratch(b, hist_bytes + thr_bytes, &d_buf));
    std::vector<int64_t> h_out(n_out);

    OrientArgs oa{};
    oa.thr = reinterpret_cast<const double *>(d_buf + hist_bytes);
    oa.box_r = s.pb.on ? s.pb.d_box : nullptr;
    oa.hist = reinterpret_cast<unsigned long long *>(d_buf);
    oa.numbins = numbins;
    oa.per_replica = per_replica ? 1 : 0;
    oa.inv_dr = (float)(1.0 / dr);
    const int64_t K = (s.n_mol + 63) / 64;
    oa.n_blocks = (int32_t)K;
    oa.tiles_per_rep = (int32_t)(K * (K + 1) / 2);
    oa.n_tiles = R * oa.tiles_per_rep;

    // waves per workgroup: as many of OR_WAVES as have room for their four rows beside the thresholds
    int nw = OR_WAVES;
    while (nw > 1 && 8 * rs + (size_t)nw * 32 * rs > OR_LDS_BYTES)
        nw >>= 1;
    const size_t lds = 8 * rs + (size_t)nw * 32 * rs;
    // persistent workgroups: four waves per SIMD of every compute unit (the pass is bound by vector
    // issue and LDS atomics), or option "wave_wgs"; no more than there are tiles
    int64_t wgs = b->wave_wgs > 0 ? b->wave_wgs : (int64_t)(16 / nw) * b->n_cus;
    wgs = std::max<int64_t>(1, std::min(wgs, (oa.n_tiles + nw - 1) / nw));

    hipStream_t st = s.stream;
    hipError_t e = hipMemsetAsync(d_buf, 0, hist_bytes, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_buf + hist_bytes, thr.data(), thr_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        if (struct_use_rec(b))
            k_orient_corr_wave<true><<<(unsigned)wgs, nw * 64, lds, st>>>(s.bv, s.rec, oa);
        else
            k_orient_corr_wave<false><<<(unsigned)wgs, nw * 64, lds, st>>>(s.bv, nullptr, oa);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(h_out.data(), d_buf, hist_bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);
    else
        (void)hipStreamSynchronize(st); // (thr and h_out of copies already queued outlive them)
    MMC_REQUIRE(e == hipSuccess, MMC_ERR_HIP, "mmc_batch_orient_corr failed: %s", hipGetErrorString(e));
    memcpy(hist, h_out.data(), hist_bytes); // (the caller's array is written only on success)
    return MMC_OK;
}
