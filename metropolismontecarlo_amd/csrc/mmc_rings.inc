// mmc_rings.inc -- host side of mmc_batch_hbond_rings (include/mmc_hip.h, "Hydrogen-bond rings"; the
// kernel is in mmc_rings.hpp).  Included by mmc_hip.hip after mmc_network.inc.
#include "mmc_rings.hpp"

#define RG_STAGE_BYTES ((size_t)256 << 20) // count_out and ring_out of one launch's replicas on the device

extern "C" int32_t mmc_batch_hbond_rings(mmc_batch *b, double r_hb, double cos_hb, int32_t n_max, int32_t per_replica,
                                         uint64_t *ring_hist, uint64_t *member_hist, int64_t *stats, uint16_t *count_out,
                                         int64_t max_rings, int32_t *ring_out)
{
    // what can be refused without the batch comes first
    MMC_REQUIRE(std::isfinite(r_hb) && r_hb > 0.0, MMC_ERR_ARG, "mmc_batch_hbond_rings: r_hb must be finite and > 0");
    MMC_REQUIRE(cos_hb > 0.0 && cos_hb <= 1.0, MMC_ERR_ARG, "mmc_batch_hbond_rings: cos_hb outside (0, 1]");
    MMC_REQUIRE(n_max >= 3 && n_max <= MMC_RING_MAX_SIZE, MMC_ERR_ARG, "mmc_batch_hbond_rings: n_max outside 3..%d",
                MMC_RING_MAX_SIZE);
    MMC_REQUIRE(ring_hist || member_hist || stats, MMC_ERR_ARG,
                "mmc_batch_hbond_rings: give at least one of ring_hist, member_hist and stats");
    MMC_REQUIRE(!ring_out || max_rings >= 1, MMC_ERR_ARG, "mmc_batch_hbond_rings: ring_out needs max_rings >= 1");
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    const int64_t R = s.R, N = s.n_mol;
    const double box_min = min_box(s);
    MMC_REQUIRE(r_hb <= box_min / 2.0, MMC_ERR_ARG, "mmc_batch_hbond_rings: r_hb = %g exceeds half of the smallest box %g",
                r_hb, box_min);
    STRUCT_STATE(b);
    BATCH_USABLE(b);
    MMC_REQUIRE(N >= 2 && N <= MMC_NET_MAX_MOL, MMC_ERR_UNSUPPORTED,
                "mmc_batch_hbond_rings: 2 .. %d molecules (a replica's graph stays in one workgroup's LDS)", MMC_NET_MAX_MOL);

    // waves per workgroup: four while four workgroups share a compute unit's LDS, eight while two do,
    // else as many of sixteen, eight or four as the device grants the level arrays of
    const size_t lds_max = (size_t)std::max<int64_t>(0, s.lds_per_block - 64);
    int nw = 4 * ring_lds((int)N, 4).bytes <= NET_LDS_PER_CU ? 4 : 2 * ring_lds((int)N, 8).bytes <= NET_LDS_PER_CU ? 8 : 16;
    while (nw > 4 && ring_lds((int)N, nw).bytes > lds_max)
        nw >>= 1;
    MMC_REQUIRE(ring_lds((int)N, nw).bytes <= lds_max, MMC_ERR_UNSUPPORTED,
                "mmc_batch_hbond_rings: the device grants %lld bytes of LDS per workgroup, %lld molecules need %zu",
                (long long)s.lds_per_block, (long long)N, ring_lds((int)N, nw).bytes + 64);
    static_assert(16 * 64 == RG_THREADS, "the largest workgroup is what k_hbond_rings is bounded for");
    const size_t lds = ring_lds((int)N, nw).bytes;

    // replicas per launch: what their count_out and ring_out leave of the staging budget
    const size_t cn_rep = count_out ? 2 * (size_t)(MMC_RING_MAX_SIZE + 1) * (size_t)N : 0,
                 rg_rep = ring_out ? 4 * (size_t)MMC_RING_MAX_SIZE * (size_t)max_rings : 0;
    int64_t chunk = cn_rep + rg_rep == 0 ? R : b->ring_chunk > 0 ? b->ring_chunk : (int64_t)(RG_STAGE_BYTES / (cn_rep + rg_rep));
    chunk = std::max<int64_t>(1, std::min(chunk, R));

    // device scratch: the histograms and stats first (zeroed), then the launch's details
    const int64_t n_rep = per_replica ? R : 1;
    const size_t rh_bytes = ring_hist ? 8 * (size_t)(n_rep * 3 * (MMC_RING_MAX_SIZE + 1)) : 0,
                 mh_bytes = member_hist ? 8 * (size_t)(n_rep * (MMC_RING_MAX_SIZE + 1) * MMC_RING_MEMBER_BINS) : 0,
                 st_bytes = 8 * (size_t)(R * MMC_RING_STATS);
    ObsCall oc(b);
    const size_t o_rh = oc.take(rh_bytes), o_mh = oc.take(mh_bytes), o_st = oc.take(st_bytes);
    const size_t o_zero_end = oc.end;
    const size_t o_cn = oc.take(cn_rep * (size_t)chunk), o_rg = oc.take(rg_rep * (size_t)chunk);
    MMC_TRY(oc.alloc());

    RingArgs ra{};
    ra.box_r = s.pb.on ? s.pb.d_box : nullptr;
    ra.ring_hist = ring_hist ? oc.at<unsigned long long>(o_rh) : nullptr;
    ra.member_hist = member_hist ? oc.at<unsigned long long>(o_mh) : nullptr;
    ra.stats = oc.at<long long>(o_st);
    ra.count = count_out ? oc.at<unsigned short>(o_cn) : nullptr;
    ra.ring = ring_out ? oc.at<int32_t>(o_rg) : nullptr;
    ra.max_rings = ring_out ? max_rings : 0;
    ra.rhb2 = r_hb * r_hb;
    ra.cos2 = cos_hb * cos_hb;
    ra.n_max = n_max;
    ra.per_replica = per_replica ? 1 : 0;

    oc.zero(o_zero_end);
    for (int64_t r0 = 0; r0 < R; r0 += chunk) {
        const int64_t nr = std::min(chunk, R - r0);
        ra.r0 = (int32_t)r0;
        ra.nr = (int32_t)nr;
        const unsigned wgs = obs_grid(b, nw, nr * nw); // a replica is a workgroup's unit
        if (oc.e == hipSuccess && ring_out) // unused rows are -1
            oc.e = hipMemsetAsync(ra.ring, 0xFF, rg_rep * (size_t)nr, oc.st);
        nbr_launch(oc, [](auto rec) { return k_hbond_rings<decltype(rec)::value>; }, wgs, (unsigned)nw * 64, lds, lds_max, ra);
        // (the copies run on the launch's stream: the next launch overwrites the staging after them)
        if (count_out)
            oc.fetch(reinterpret_cast<char *>(count_out) + cn_rep * (size_t)r0, oc.at<char>(o_cn), cn_rep * (size_t)nr);
        if (ring_out)
            oc.fetch(reinterpret_cast<char *>(ring_out) + rg_rep * (size_t)r0, oc.at<char>(o_rg), rg_rep * (size_t)nr);
    }
    oc.fetch(ring_hist, oc.at<char>(o_rh), rh_bytes);
    oc.fetch(member_hist, oc.at<char>(o_mh), mh_bytes);
    oc.fetch(stats, oc.at<char>(o_st), st_bytes);
    return oc.finish("mmc_batch_hbond_rings");
}
