// mmc_orient.inc -- host side of mmc_batch_orient_corr (include/mmc_hip.h, "Orientational pair
// correlations"; the kernel is in mmc_orient.hpp).  Included by mmc_hip.hip after mmc_units.inc
// (ObsCall, tile_plan: the bins are mmc_batch_rdf_sites').
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
    OrientArgs oa{};
    std::vector<double> thr;
    MMC_TRY(tile_plan(b, numbins, r_max, "mmc_batch_orient_corr", &oa.ta, &thr));
    oa.ta.per_replica = per_replica ? 1 : 0;

    // waves per workgroup: the thresholds, and four 64-bit rows a wave
    const size_t rs = (size_t)numbins + 2;
    const int nw = tile_waves(8 * rs, 32 * rs);
    const size_t lds = 8 * rs + (size_t)nw * 32 * rs;
    const unsigned wgs = obs_grid(b, nw, oa.ta.n_tiles);

    ObsCall oc(b);
    const size_t hist_bytes = sizeof(unsigned long long) * (size_t)(per_replica ? s.R : 1) * 4 * rs;
    const size_t o_hist = oc.take(hist_bytes), o_thr = oc.take(sizeof(double) * thr.size());
    MMC_TRY(oc.alloc());
    oa.hist = oc.at<unsigned long long>(o_hist);
    oa.ta.thr = oc.at<double>(o_thr);
    oc.zero(hist_bytes);
    oc.to_device(oc.at<double>(o_thr), thr.data(), sizeof(double) * thr.size());
    if (oc.e == hipSuccess) {
        if (struct_use_rec(b))
            k_orient_corr_wave<true><<<wgs, nw * 64, lds, oc.st>>>(s.bv, s.rec, oa);
        else
            k_orient_corr_wave<false><<<wgs, nw * 64, lds, oc.st>>>(s.bv, nullptr, oa);
    }
    oc.launched();
    oc.fetch(hist, oa.hist, hist_bytes);
    return oc.finish("mmc_batch_orient_corr");
}
