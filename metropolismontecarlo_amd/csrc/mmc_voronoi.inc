// mmc_voronoi.inc -- host side of mmc_batch_voronoi (include/mmc_hip.h, "Voronoi cells"; the kernels
// are in mmc_voronoi.hpp).  Included by mmc_hip.hip after mmc_shell.inc.
#include "mmc_voronoi.hpp"

static_assert(MMC_VORONOI_CAP == MMC_SHELL_CAP && MMC_VORONOI_CAP == 64, "the list of mmc_batch_shell_order: one lane per neighbour");

extern "C" int32_t mmc_batch_voronoi(mmc_batch *b, double r_list, double area_min, int32_t v_bins, double v_max,
                                     int32_t eta_bins, double eta_max, int32_t r_bins, int32_t per_replica,
                                     uint64_t *vol_hist, uint64_t *eta_hist, uint64_t *face_hist, uint64_t *side_hist,
                                     uint64_t *nbr_hist, uint64_t *flagged, double *sums, double *vol_out, double *area_out,
                                     int32_t *faces_out, int32_t *nbr_out, double *face_area_out)
{
    // what can be refused without the batch comes first
    MMC_REQUIRE(std::isfinite(r_list) && r_list > 0.0, MMC_ERR_ARG, "mmc_batch_voronoi: r_list must be finite and > 0");
    MMC_REQUIRE(std::isfinite(area_min) && area_min >= 0.0, MMC_ERR_ARG, "mmc_batch_voronoi: area_min must be finite and >= 0");
    MMC_REQUIRE(v_bins >= 1 && v_bins <= MMC_VORONOI_MAX_BINS, MMC_ERR_ARG, "mmc_batch_voronoi: v_bins outside 1..%d",
                MMC_VORONOI_MAX_BINS);
    MMC_REQUIRE(std::isfinite(v_max) && v_max > 0.0, MMC_ERR_ARG, "mmc_batch_voronoi: v_max must be finite and > 0");
    MMC_REQUIRE(eta_bins >= 1 && eta_bins <= MMC_VORONOI_MAX_BINS, MMC_ERR_ARG, "mmc_batch_voronoi: eta_bins outside 1..%d",
                MMC_VORONOI_MAX_BINS);
    MMC_REQUIRE(std::isfinite(eta_max) && eta_max > 1.0, MMC_ERR_ARG, "mmc_batch_voronoi: eta_max must be finite and > 1");
    MMC_REQUIRE(r_bins >= 1 && r_bins <= MMC_VORONOI_MAX_BINS, MMC_ERR_ARG, "mmc_batch_voronoi: r_bins outside 1..%d",
                MMC_VORONOI_MAX_BINS);
    MMC_REQUIRE(vol_hist || eta_hist || face_hist || side_hist || nbr_hist || flagged || sums || vol_out || area_out ||
                    faces_out || nbr_out || face_area_out,
                MMC_ERR_ARG, "mmc_batch_voronoi: give at least one output");
    // a workgroup's counters: the three flags, then the histograms that are asked for (at most
    // 3 + 3 x 1025 + 65 + 17 words: the bounds on the bins keep them beside one wave's list and polygons)
    const size_t w_vol = vol_hist ? (size_t)v_bins + 1 : 0, w_eta = eta_hist ? (size_t)eta_bins + 1 : 0,
                 w_face = face_hist ? MMC_VORONOI_CAP + 1 : 0, w_side = side_hist ? MMC_VORONOI_MAXV + 1 : 0,
                 w_nbr = nbr_hist ? (size_t)r_bins + 1 : 0;
    const size_t hs = 3 + w_vol + w_eta + w_face + w_side + w_nbr;
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    const int64_t R = s.R, N = s.n_mol;
    const double box_min = min_box(s);
    MMC_REQUIRE(r_list <= box_min / 2.0, MMC_ERR_ARG, "mmc_batch_voronoi: r_list %g exceeds half of the smallest box %g",
                r_list, box_min);
    STRUCT_STATE(b);
    BATCH_USABLE(b);
    MMC_REQUIRE(N >= 2 && N <= (1 << 21), MMC_ERR_UNSUPPORTED, "mmc_batch_voronoi: 2 .. 2^21 molecules");

    // waves per workgroup: as many of VO_WAVES as the device's LDS holds beside the counters and the
    // staged O positions (one workgroup per compute unit then); without staging where even one does not
    const size_t lds_max = (size_t)std::max<int64_t>(0, s.lds_per_block - 64), per_wave = NBR_LIST_BYTES + VO_POLY_BYTES;
    auto lds_of = [&](int nw, bool st) { return (((size_t)nw * per_wave + 4 * hs + 15) & ~(size_t)15) + (st ? 24 * (size_t)N : 0); };
    const bool stage = stage_fits(b, lds_of(1, false), N, lds_max);
    int nw = VO_WAVES;
    while (nw > 1 && lds_of(nw, stage) > lds_max)
        nw--;
    const size_t lds = lds_of(nw, stage);
    MMC_REQUIRE(lds <= lds_max, MMC_ERR_UNSUPPORTED, "mmc_batch_voronoi: %zu bytes of LDS for one wave exceed the device's %lld",
                lds + 64, (long long)s.lds_per_block);

    // device scratch: the counters first (zeroed), then what is asked for per molecule
    const int64_t n_rep = per_replica ? R : 1;
    const bool want_pm = sums || vol_out || area_out || faces_out;
    const size_t fl_bytes = 8 * 3 * (size_t)R, vh_bytes = 8 * (size_t)n_rep * w_vol, eh_bytes = 8 * (size_t)n_rep * w_eta,
                 fh_bytes = 8 * (size_t)n_rep * w_face, sh_bytes = 8 * (size_t)n_rep * w_side, nh_bytes = 8 * (size_t)n_rep * w_nbr;
    const size_t sm_bytes = 64 * (size_t)R, pm_bytes = 8 * (size_t)(R * N), ft_bytes = 4 * (size_t)(R * N),
                 nb_bytes = 4 * (size_t)MMC_VORONOI_CAP * (size_t)(R * N), fa_bytes = 8 * (size_t)MMC_VORONOI_CAP * (size_t)(R * N);
    ObsCall oc(b);
    const size_t o_fl = oc.take(fl_bytes), o_vh = oc.take(vh_bytes), o_eh = oc.take(eh_bytes), o_fh = oc.take(fh_bytes),
                 o_sh = oc.take(sh_bytes), o_nh = oc.take(nh_bytes);
    const size_t o_zero_end = oc.end;
    const size_t o_sm = oc.take(sums ? sm_bytes : 0), o_vo = oc.take(want_pm ? pm_bytes : 0), o_ar = oc.take(want_pm ? pm_bytes : 0),
                 o_ca = oc.take(sums ? pm_bytes : 0), o_ft = oc.take(want_pm ? ft_bytes : 0),
                 o_nb = oc.take(nbr_out ? nb_bytes : 0), o_fa = oc.take(face_area_out ? fa_bytes : 0);
    MMC_TRY(oc.alloc());

    VoronoiArgs va{};
    va.box_r = s.pb.on ? s.pb.d_box : nullptr;
    va.flagged = oc.at<unsigned long long>(o_fl);
    va.vol_hist = vol_hist ? oc.at<unsigned long long>(o_vh) : nullptr;
    va.eta_hist = eta_hist ? oc.at<unsigned long long>(o_eh) : nullptr;
    va.face_hist = face_hist ? oc.at<unsigned long long>(o_fh) : nullptr;
    va.side_hist = side_hist ? oc.at<unsigned long long>(o_sh) : nullptr;
    va.nbr_hist = nbr_hist ? oc.at<unsigned long long>(o_nh) : nullptr;
    va.vol = want_pm ? oc.at<double>(o_vo) : nullptr;
    va.area = want_pm ? oc.at<double>(o_ar) : nullptr;
    va.carea = sums ? oc.at<double>(o_ca) : nullptr;
    va.faces = want_pm ? oc.at<int32_t>(o_ft) : nullptr;
    va.nbr = nbr_out ? oc.at<int32_t>(o_nb) : nullptr;
    va.face_area = face_area_out ? oc.at<double>(o_fa) : nullptr;
    va.rl = r_list;
    va.rl2 = r_list * r_list;
    va.area_min = area_min;
    va.v_scale = v_bins / v_max;
    va.eta_scale = eta_bins / (eta_max - 1.0);
    va.inv_dr = r_bins / r_list;
    va.k36pi = 36.0 * 3.141592653589793;
    va.v_bins = v_bins;
    va.eta_bins = eta_bins;
    va.r_bins = r_bins;
    va.o_eta = (int32_t)(3 + w_vol);
    va.o_face = (int32_t)(va.o_eta + w_eta);
    va.o_side = (int32_t)(va.o_face + w_face);
    va.o_nbr = (int32_t)(va.o_side + w_side);
    va.hs = (int32_t)hs;
    va.per_replica = per_replica ? 1 : 0;
    va.R = (int32_t)R;
    va.prune = b->voronoi_prune;

    // persistent workgroups: as many as are resident (the LDS decides), or option "wave_wgs"; no more
    // than give every wave a molecule
    const int64_t resident = std::max<int64_t>(1, (int64_t)(VO_CU_LDS / (lds + 64))) * b->n_cus;
    const int64_t want = b->wave_wgs > 0 ? b->wave_wgs : resident;
    const unsigned g = (unsigned)std::max<int64_t>(1, std::min(want, (R * N + nw - 1) / nw)), t = (unsigned)nw * 64;

    oc.zero(o_zero_end); // every counter
    nbr_launch(oc, [](auto rec, auto st) { return k_voronoi_wave<decltype(rec)::value, decltype(st)::value>; }, stage, g, t, lds,
               lds_max, va);
    if (oc.e == hipSuccess && sums)
        k_voronoi_sums<<<(unsigned)((R + NBR_WAVES - 1) / NBR_WAVES), NBR_WAVES * 64, 0, oc.st>>>(
            va.vol, va.area, va.carea, va.faces, va.k36pi, oc.at<double>(o_sm), (int)N, (int)R);
    oc.launched();
    oc.fetch(flagged, oc.at<char>(o_fl), fl_bytes);
    oc.fetch(vol_hist, oc.at<char>(o_vh), vh_bytes);
    oc.fetch(eta_hist, oc.at<char>(o_eh), eh_bytes);
    oc.fetch(face_hist, oc.at<char>(o_fh), fh_bytes);
    oc.fetch(side_hist, oc.at<char>(o_sh), sh_bytes);
    oc.fetch(nbr_hist, oc.at<char>(o_nh), nh_bytes);
    oc.fetch(sums, oc.at<char>(o_sm), sm_bytes);
    oc.fetch(vol_out, oc.at<char>(o_vo), pm_bytes);
    oc.fetch(area_out, oc.at<char>(o_ar), pm_bytes);
    oc.fetch(faces_out, oc.at<char>(o_ft), ft_bytes);
    oc.fetch(nbr_out, oc.at<char>(o_nb), nb_bytes);
    oc.fetch(face_area_out, oc.at<char>(o_fa), fa_bytes);
    return oc.finish("mmc_batch_voronoi");
}
