// mmc_network.inc -- host side of mmc_batch_hbond_network (include/mmc_hip.h, "Hydrogen-bond
// network"; the kernel is in mmc_network.hpp).  Included by mmc_hip.hip after mmc_units.inc (ObsCall).
#include "mmc_network.hpp"

#define NET_LDS_PER_CU 163840 // what the workgroups resident on a gfx950 compute unit share

extern "C" int32_t mmc_batch_hbond_network(mmc_batch *b, int32_t n_crit, const double *r_hb, const double *cos_hb,
                                           const int32_t *min_bonds, int32_t per_replica, uint64_t *size_hist,
                                           uint64_t *deg_hist, int64_t *stats, int32_t *label_out, int32_t *nbr_out)
{
    // what can be refused without the batch comes first
    MMC_REQUIRE(n_crit >= 1 && n_crit <= MMC_NET_MAX_CRIT, MMC_ERR_ARG,
                "mmc_batch_hbond_network: n_crit outside 1..%d", MMC_NET_MAX_CRIT);
    MMC_REQUIRE(r_hb && cos_hb && min_bonds, MMC_ERR_ARG, "mmc_batch_hbond_network: %s is NULL",
                !r_hb ? "r_hb" : !cos_hb ? "cos_hb" : "min_bonds");
    for (int k = 0; k < n_crit; k++) {
        MMC_REQUIRE(std::isfinite(r_hb[k]) && r_hb[k] > 0.0, MMC_ERR_ARG,
                    "mmc_batch_hbond_network: r_hb[%d] must be finite and > 0", k);
        MMC_REQUIRE(cos_hb[k] > 0.0 && cos_hb[k] <= 1.0, MMC_ERR_ARG,
                    "mmc_batch_hbond_network: cos_hb[%d] outside (0, 1]", k);
        MMC_REQUIRE(min_bonds[k] >= 0 && min_bonds[k] <= MMC_NET_MAX_DEG, MMC_ERR_ARG,
                    "mmc_batch_hbond_network: min_bonds[%d] outside 0..%d", k, MMC_NET_MAX_DEG);
    }
    MMC_REQUIRE(size_hist || deg_hist || stats, MMC_ERR_ARG,
                "mmc_batch_hbond_network: give at least one of size_hist, deg_hist and stats");
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    const int64_t R = s.R, N = s.n_mol, K = n_crit;
    const double box_min = min_box(s);
    for (int k = 0; k < n_crit; k++)
        MMC_REQUIRE(r_hb[k] <= box_min / 2.0, MMC_ERR_ARG,
                    "mmc_batch_hbond_network: r_hb[%d] = %g exceeds half of the smallest box %g", k, r_hb[k], box_min);
    STRUCT_STATE(b);
    BATCH_USABLE(b);
    MMC_REQUIRE(N >= 2 && N <= MMC_NET_MAX_MOL, MMC_ERR_UNSUPPORTED,
                "mmc_batch_hbond_network: 2 .. %d molecules (a replica's graph stays in one workgroup's LDS)",
                MMC_NET_MAX_MOL);
    // (a batch holds three-atom molecules only, mmc_batch_create: slots 0..2 exist in every molecule)

    // criteria per pass over the molecules: as many as the LDS holds lists of, then evened out over
    // the passes; and as many waves as share a compute unit's LDS sixteen at a time (as mmc_batch_sdf)
    const size_t lds_max = (size_t)std::max<int64_t>(0, s.lds_per_block - 64);
    int group = n_crit;
    while (group > 1 && net_lds((int)N, group, 16).bytes > lds_max)
        group--;
    MMC_REQUIRE(net_lds((int)N, group, 16).bytes <= lds_max, MMC_ERR_UNSUPPORTED,
                "mmc_batch_hbond_network: the device grants %lld bytes of LDS per workgroup, %lld molecules need %zu",
                (long long)s.lds_per_block, (long long)N, net_lds((int)N, 1, 16).bytes + 64);
    const int passes = (n_crit + group - 1) / group;
    group = (n_crit + passes - 1) / passes;
    const int per_cu = (int)std::min<size_t>(4, NET_LDS_PER_CU / net_lds((int)N, group, 16).bytes);
    const int nw = per_cu >= 4 ? 4 : per_cu >= 2 ? 8 : 16;
    static_assert(16 * 64 == NET_THREADS, "the largest workgroup is what k_hbond_network is bounded for");
    const size_t lds = net_lds((int)N, group, nw).bytes;
    const unsigned wgs = obs_grid(b, nw, R * nw); // a replica is a workgroup's unit

    // device scratch: the histograms first (zeroed), then the rest
    const int64_t n_rep = per_replica ? R : 1;
    const size_t sh_bytes = size_hist ? 8 * (size_t)(n_rep * K * (N + 1)) : 0,
                 dh_bytes = deg_hist ? 8 * (size_t)(n_rep * K * (MMC_NET_MAX_DEG + 1)) : 0,
                 st_bytes = 8 * (size_t)(R * K * MMC_NET_STATS), lb_bytes = label_out ? 4 * (size_t)(R * K * N) : 0,
                 nb_bytes = nbr_out ? 4 * (size_t)(R * K * N * MMC_NET_MAX_DEG) : 0;
    ObsCall oc(b);
    const size_t o_sh = oc.take(sh_bytes), o_dh = oc.take(dh_bytes), o_st = oc.take(st_bytes), o_lb = oc.take(lb_bytes),
                 o_nb = oc.take(nb_bytes);
    MMC_TRY(oc.alloc());

    NetArgs na{};
    na.box_r = s.pb.on ? s.pb.d_box : nullptr;
    na.size_hist = size_hist ? oc.at<unsigned long long>(o_sh) : nullptr;
    na.deg_hist = deg_hist ? oc.at<unsigned long long>(o_dh) : nullptr;
    na.stats = oc.at<long long>(o_st);
    na.label = label_out ? oc.at<int32_t>(o_lb) : nullptr;
    na.nbr = nbr_out ? oc.at<int32_t>(o_nb) : nullptr;
    for (int k = 0; k < n_crit; k++) {
        na.rhb2[k] = r_hb[k] * r_hb[k];
        na.cos2[k] = cos_hb[k] * cos_hb[k];
        na.min_bonds[k] = min_bonds[k];
    }
    na.n_crit = n_crit;
    na.group = group;
    na.per_replica = per_replica ? 1 : 0;
    na.R = (int32_t)R;

    if (o_st > 0)
        oc.zero(o_st);
    nbr_launch(oc, [](auto rec) { return k_hbond_network<decltype(rec)::value>; }, wgs, (unsigned)nw * 64, lds, lds_max, na);
    oc.fetch(size_hist, oc.at<char>(o_sh), sh_bytes);
    oc.fetch(deg_hist, oc.at<char>(o_dh), dh_bytes);
    oc.fetch(stats, oc.at<char>(o_st), st_bytes);
    oc.fetch(label_out, oc.at<char>(o_lb), lb_bytes);
    oc.fetch(nbr_out, oc.at<char>(o_nb), nb_bytes);
    return oc.finish("mmc_batch_hbond_network");
}
