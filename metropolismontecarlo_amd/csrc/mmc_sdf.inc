// mmc_sdf.inc -- host side of mmc_batch_sdf (include/mmc_hip.h, "Spatial distribution functions";
// the kernel is in mmc_sdf.hpp).  Included by mmc_hip.hip after mmc_units.inc (ObsCall).
#include "mmc_sdf.hpp"

#define SDF_LDS_PER_CU 163840 // what the workgroups resident on a gfx950 compute unit share

extern "C" int32_t mmc_batch_sdf(mmc_batch *b, int32_t n_half, double cell, int32_t fold, int32_t site_mask,
                                 int32_t per_replica, uint64_t *hist)
{
    // what can be refused without the batch comes first
    MMC_REQUIRE(hist, MMC_ERR_ARG, "mmc_batch_sdf: NULL out pointer");
    MMC_REQUIRE(n_half >= 1, MMC_ERR_ARG, "mmc_batch_sdf: n_half must be >= 1");
    MMC_REQUIRE(std::isfinite(cell) && cell > 0.0, MMC_ERR_ARG, "mmc_batch_sdf: cell must be finite and > 0");
    MMC_REQUIRE(fold >= 0 && fold <= 3, MMC_ERR_ARG, "mmc_batch_sdf: fold outside 0..3");
    MMC_REQUIRE(site_mask >= 1 && site_mask <= 7, MMC_ERR_ARG, "mmc_batch_sdf: site_mask outside 1..7");
    // g_x g_y g_z >= 2 n_half^3: beyond 25 it is refused whatever the fold, and below the product is small
    const int64_t gx = (fold & 1) ? n_half : 2 * (int64_t)n_half, gy = (fold & 2) ? n_half : 2 * (int64_t)n_half,
                  gz = 2 * (int64_t)n_half;
    MMC_REQUIRE(n_half <= 25 && gx * gy * gz <= MMC_SDF_MAX_CELLS, MMC_ERR_ARG,
                "mmc_batch_sdf: the grid has more than %d cells", MMC_SDF_MAX_CELLS);
    const int64_t n_cells = gx * gy * gz;
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    STRUCT_STATE(b);
    // the cube against the periodic images: rho = 2 r_mol_max bounds every |o_a|
    const double min_box = s.pb.on ? *std::min_element(s.pb.box.begin(), s.pb.box.end()) : s.bv.box;
    const double reach = std::sqrt(3.0) * n_half * cell + 2.0 * s.r_mol_max;
    MMC_REQUIRE(reach <= min_box / 2.0, MMC_ERR_ARG, // (false for an r_mol_max that is not known)
                "mmc_batch_sdf: sqrt(3) n_half cell + 2 r_mol_max = %g exceeds half of the smallest box %g", reach,
                min_box);
    MMC_REQUIRE(s.n_mol >= 1 && s.n_mol <= (1 << 21), MMC_ERR_UNSUPPORTED,
                "mmc_batch_sdf: 1 .. 2^21 molecules (the tiles of a replica are counted in 32 bits)");
    // (a batch holds three-atom molecules only, mmc_batch_create: slots 0..2 exist in every molecule)
    const int n_edge = 2 * n_half + 1;
    const size_t lds = 8 * (size_t)n_edge + 4 * (size_t)n_cells;
    MMC_REQUIRE((int64_t)lds + 64 <= s.lds_per_block, MMC_ERR_UNSUPPORTED,
                "mmc_batch_sdf: the device grants %lld bytes of LDS per workgroup, %lld cells need %zu",
                (long long)s.lds_per_block, (long long)n_cells, lds + 64);

    SdfArgs sa{};
    const int64_t K = (s.n_mol + 63) / 64;
    sa.ta.box_r = s.pb.on ? s.pb.d_box : nullptr;
    sa.ta.per_replica = per_replica ? 1 : 0;
    sa.ta.n_blocks = (int32_t)K;
    sa.ta.tiles_per_rep = (int32_t)(K * (K + 1) / 2);
    sa.ta.n_tiles = s.R * sa.ta.tiles_per_rep;
    sa.n_half = n_half;
    sa.fold = fold;
    sa.site_mask = site_mask;
    sa.n_cells = (int32_t)n_cells;
    sa.inv_cell = (float)(1.0 / cell);
    std::vector<double> edge((size_t)n_edge);
    for (int k = -n_half; k <= n_half; k++)
        edge[(size_t)(k + n_half)] = (double)k * cell;

    // Sixteen waves per compute unit, four per SIMD, in as many workgroups as its LDS holds grids:
    // 4 x 4 waves up to 40 KB a grid, 2 x 8 up to 80 KB, then one workgroup of 16.  Or option "wave_wgs".
    const int per_cu = (int)std::min<size_t>(4, SDF_LDS_PER_CU / lds), nw = per_cu >= 4 ? 4 : per_cu >= 2 ? 8 : 16;
    static_assert(16 * 64 == SDF_THREADS, "the largest workgroup is what k_sdf_wave is bounded for");
    const int64_t want = b->wave_wgs > 0 ? b->wave_wgs : (int64_t)(16 / nw) * std::max(1, b->n_cus);
    const unsigned wgs = (unsigned)std::max<int64_t>(1, std::min(want, (sa.ta.n_tiles + nw - 1) / nw));

    ObsCall oc(b);
    const size_t hist_bytes = sizeof(unsigned long long) * (size_t)(per_replica ? s.R : 1) * (size_t)(n_cells + 2);
    const size_t o_hist = oc.take(hist_bytes), o_edge = oc.take(sizeof(double) * edge.size());
    MMC_TRY(oc.alloc());
    sa.hist = oc.at<unsigned long long>(o_hist);
    sa.ta.thr = oc.at<double>(o_edge);
    const bool use_rec = struct_use_rec(b);
    if (lds > TILE_LDS_BYTES) // beyond what a workgroup may ask for without opting in: as k_sofq_wave
        oc.e = hipFuncSetAttribute(use_rec ? reinterpret_cast<const void *>(k_sdf_wave<true>)
                                           : reinterpret_cast<const void *>(k_sdf_wave<false>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)(s.lds_per_block - 64));
    oc.zero(hist_bytes);
    oc.to_device(oc.at<double>(o_edge), edge.data(), sizeof(double) * edge.size());
    if (oc.e == hipSuccess) {
        if (use_rec)
            k_sdf_wave<true><<<wgs, nw * 64, lds, oc.st>>>(s.bv, s.rec, sa);
        else
            k_sdf_wave<false><<<wgs, nw * 64, lds, oc.st>>>(s.bv, nullptr, sa);
    }
    oc.launched();
    oc.fetch(hist, sa.hist, hist_bytes);
    return oc.finish("mmc_batch_sdf");
}
