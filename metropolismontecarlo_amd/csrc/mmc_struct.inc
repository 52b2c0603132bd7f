// mmc_struct.inc -- host side of the structure observables (include/mmc_hip.h, "Structure
// observables"; the kernels are in mmc_struct.hpp).  Included by mmc_hip.hip after mmc_units.inc
// (ObsCall, tile_plan).
#include "mmc_struct.hpp"

extern "C" int32_t mmc_batch_rdf_sites(mmc_batch *b, int32_t numbins, double r_max, int32_t per_replica,
                                       uint64_t *hist)
{
    // what can be refused without the batch comes first
    MMC_REQUIRE(hist, MMC_ERR_ARG, "mmc_batch_rdf_sites: NULL out pointer");
    MMC_REQUIRE(numbins >= 1 && numbins <= MMC_RDF_SITES_MAX_BINS, MMC_ERR_ARG,
                "mmc_batch_rdf_sites: numbins outside 1..%d", MMC_RDF_SITES_MAX_BINS);
    MMC_REQUIRE(std::isfinite(r_max), MMC_ERR_ARG, "mmc_batch_rdf_sites: r_max is not finite");
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    RdfSitesArgs sa{};
    std::vector<double> thr;
    MMC_TRY(tile_plan(b, numbins, r_max, "mmc_batch_rdf_sites", &sa.ta, &thr));
    sa.ta.per_replica = per_replica ? 1 : 0;

    // waves per workgroup: the thresholds, and six 32-bit rows a wave
    const size_t rs = (size_t)numbins + 2;
    const int nw = tile_waves(8 * rs, 24 * rs);
    const size_t lds = 8 * rs + (size_t)nw * 24 * rs;
    const unsigned wgs = obs_grid(b, nw, sa.ta.n_tiles);

    ObsCall oc(b);
    const size_t hist_bytes = sizeof(unsigned long long) * (size_t)(per_replica ? s.R : 1) * 6 * (size_t)(numbins + 1);
    const size_t o_hist = oc.take(hist_bytes), o_thr = oc.take(sizeof(double) * thr.size());
    MMC_TRY(oc.alloc());
    sa.hist = oc.at<unsigned long long>(o_hist);
    sa.ta.thr = oc.at<double>(o_thr);
    oc.zero(hist_bytes);
    oc.to_device(oc.at<double>(o_thr), thr.data(), sizeof(double) * thr.size());
    if (oc.e == hipSuccess) {
        if (struct_use_rec(b))
            k_rdf_sites_wave<true><<<wgs, nw * 64, lds, oc.st>>>(s.bv, s.rec, sa);
        else
            k_rdf_sites_wave<false><<<wgs, nw * 64, lds, oc.st>>>(s.bv, nullptr, sa);
    }
    oc.launched();
    oc.fetch(hist, sa.hist, hist_bytes);
    return oc.finish("mmc_batch_rdf_sites");
}

extern "C" int32_t mmc_batch_dipoles(mmc_batch *b, double *dip)
{
    MMC_REQUIRE(dip, MMC_ERR_ARG, "mmc_batch_dipoles: NULL out pointer");
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    const int64_t R = s.R;
    STRUCT_STATE(b);
    ObsCall oc(b);
    const size_t bytes = sizeof(double) * 3 * (size_t)R, o_dip = oc.take(bytes);
    MMC_TRY(oc.alloc());
    double *d_dip = oc.at<double>(o_dip);
    const unsigned wgs = (unsigned)((R + ST_WAVES - 1) / ST_WAVES);
    const double *box_r = s.pb.on ? s.pb.d_box : nullptr;
    if (struct_use_rec(b))
        k_dipoles<true><<<wgs, ST_WAVES * 64, 0, oc.st>>>(s.bv, s.rec, box_r, d_dip, (int)R);
    else
        k_dipoles<false><<<wgs, ST_WAVES * 64, 0, oc.st>>>(s.bv, nullptr, box_r, d_dip, (int)R);
    oc.launched();
    oc.fetch(dip, d_dip, bytes);
    return oc.finish("mmc_batch_dipoles");
}
