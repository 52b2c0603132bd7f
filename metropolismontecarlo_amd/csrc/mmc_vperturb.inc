// mmc_vperturb.inc -- host side of mmc_batch_volume_perturb (include/mmc_hip.h, "Virtual volume
// moves"; the kernels are in mmc_vperturb.hpp).  Included by mmc_hip.hip after mmc_units.inc (ObsCall)
// and mmc_perbox.inc, whose domain rule it shares.
#include "mmc_vperturb.hpp"

#define VP_PARTS_BYTES ((size_t)256 << 20) // tile-pair partials of one chunk of replicas

extern "C" int32_t mmc_batch_volume_perturb(mmc_batch *b, int32_t n_scale, const double *scale,
                                            double temperature, double *boltz_sum, int64_t *n_overlap,
                                            double *du_out, double *base_out)
{
    // what can be refused without the batch comes first
    MMC_REQUIRE(n_scale >= 1 && n_scale <= VP_MAX_SCALES, MMC_ERR_ARG,
                "mmc_batch_volume_perturb: n_scale outside 1..%d", VP_MAX_SCALES);
    MMC_REQUIRE(scale, MMC_ERR_ARG, "mmc_batch_volume_perturb: scale is NULL");
    for (int k = 0; k < n_scale; k++)
        MMC_REQUIRE(std::isfinite(scale[k]) && scale[k] > 0.0, MMC_ERR_ARG,
                    "mmc_batch_volume_perturb: scale[%d] must be finite and > 0", k);
    MMC_REQUIRE(std::isfinite(temperature) && temperature > 0.0, MMC_ERR_ARG,
                "mmc_batch_volume_perturb: temperature must be finite and > 0");
    MMC_REQUIRE(boltz_sum || n_overlap || du_out || base_out, MMC_ERR_ARG,
                "mmc_batch_volume_perturb: give at least one of boltz_sum, n_overlap, du_out and base_out");
    BATCH_CHECK(b);
    STRUCT_STATE(b);
    BATCH_USABLE(b);
    BATCH_NOT_WOLF(b, "mmc_batch_volume_perturb");
    BATCH_ONE_BOX(b, "mmc_batch_volume_perturb");
    BATCH_NO_SOLUTE(b, "mmc_batch_volume_perturb");
    DeviceSystem &s = b->sys;
    MMC_REQUIRE(s.uploaded && s.ewald_ready, MMC_ERR_STATE,
                "mmc_batch_volume_perturb needs an uploaded system and PrepareEwaldVariables");
    const int64_t R = s.R, N = s.n_mol;
    const int n_box = n_scale + 1;
    const double L = s.bv.box, alpha = s.bv.kappa * L; // main.jl:290-291
    VpArgs va{};
    va.n_box = n_box;
    double min_box = INFINITY;
    for (int k = 0; k < n_box; k++) {
        va.f[k] = k == 0 ? 1.0 : scale[k - 1];
        va.box[k] = va.f[k] * L;
        va.kappa[k] = alpha / va.box[k];
        MMC_REQUIRE(pb_box_ok(b, va.box[k]), MMC_ERR_ARG,
                    "mmc_batch_volume_perturb: test box %g (scale %g) is below 2 r_cut", va.box[k], va.f[k]);
        min_box = std::min(min_box, va.box[k]);
    }
    {   // the pb_domain_ok condition at the smallest test box, and records kept in step with the moves
        const double kappa = alpha / min_box, slack = b->qq_rcut * b->qq_rcut + 100; // ewalds.jl:362
        MMC_REQUIRE(s.homogeneous && s.rec && b->fast_ok && N <= MMC_WAVE_MAX_MOL && kappa <= MMC_QQ_KAPPA_MAX
                        && slack <= MMC_QQ_UMAX && kappa * std::sqrt(slack) <= MMC_QQ_XMAX,
                    MMC_ERR_UNSUPPORTED,
                    "mmc_batch_volume_perturb: the erfc table does not cover kappa = alpha / L_min = %.4g "
                    "(needs kappa <= %.2f and kappa * sqrt(r_cut^2 + 100) <= %.1f, identical 3-atom molecules)",
                    kappa, MMC_QQ_KAPPA_MAX, MMC_QQ_XMAX);
    }
    // k_vp_recip keeps a replica's phases, charges and S(k) in one workgroup's LDS
    const size_t lds = sizeof(double) * (7 * (size_t)s.n_atoms + (s.n_atoms & 1) + 2 * MMC_NK_STRIDE);
    MMC_REQUIRE((int64_t)lds + 256 <= s.lds_per_block, MMC_ERR_UNSUPPORTED,
                "mmc_batch_volume_perturb: at most %lld atoms (a replica's phases in one "
                "workgroup's LDS)", (long long)((s.lds_per_block - 256) / 8 - 2 * MMC_NK_STRIDE) / 7);
    MMC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_vp_recip),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)(s.lds_per_block - 256)));
    double sq, sq2;
    MMC_TRY(s.charge_sums(&sq, &sq2));

    // device scratch: box scalars, cfac rows and tables of this call, then results
    const int n_pairs = s.n_tile_pairs;
    int64_t chunk = (int64_t)(VP_PARTS_BYTES / (sizeof(VpPart) * (size_t)n_box * n_pairs));
    chunk = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(chunk, R), 32768));
    const size_t sm_bytes = sizeof(VpPart) * (size_t)R * n_box, er_bytes = sizeof(double) * (size_t)R * n_box;
    ObsCall oc(b);
    const size_t o_sc = oc.take(sizeof(double) * 2 * VP_BOXES), o_cf = oc.take(sizeof(double) * MMC_NK_STRIDE * VP_BOXES),
                 o_tb = oc.take(sizeof(double) * MMC_QQ_TABLE_DOUBLES * VP_BOXES),
                 o_pt = oc.take(sizeof(VpPart) * (size_t)chunk * n_box * n_pairs), o_sm = oc.take(sm_bytes),
                 o_er = oc.take(er_bytes);
    MMC_TRY(oc.alloc());
    double *d_kappa = oc.at<double>(o_sc), *d_box = d_kappa + VP_BOXES;
    double *d_cfac = oc.at<double>(o_cf), *d_tabs = oc.at<double>(o_tb), *d_erec = oc.at<double>(o_er);
    VpPart *d_parts = oc.at<VpPart>(o_pt), *d_sums = oc.at<VpPart>(o_sm);

    hipStream_t st = oc.st;
    oc.to_device(d_kappa, va.kappa, sizeof(double) * VP_BOXES);
    oc.to_device(d_box, va.box, sizeof(double) * VP_BOXES);
    if (oc.e == hipSuccess) { // PrepareEwaldVariables at (kappa_k, L_k) over the batch's k list (ewalds.jl:45-103)
        k_cfac_pb<<<dim3((unsigned)((s.nkvecs + 63) / 64), (unsigned)n_box), 64, 0, st>>>(
            s.bv.kxyz, (int)s.nkvecs, d_kappa, d_box, d_cfac, nullptr, s.half_k ? 1 : 0);
        k_build_qq_table<<<dim3((MMC_QQ_NROW + 63) / 64, (unsigned)n_box), 64, 0, st>>>(
            0.0, d_tabs, PerBoxTable{ d_kappa, nullptr });
    }
    oc.launched();
    const PairParams pp = mmc_pair_params(b->lj_rcut, b->qq_rcut, 0.0, 0.5, s.bv.kappa, false);
    for (int64_t r0 = 0; r0 < R && oc.e == hipSuccess; r0 += chunk) {
        const int64_t nr = std::min(chunk, R - r0);
        va.r0 = (int32_t)r0;
        k_vp_pairs<<<dim3((unsigned)n_pairs, (unsigned)nr), MMC_BLOCK, 0, st>>>(
            s.bv, s.rec, d_tabs, s.fc, pp, va, s.tile_pairs, n_pairs, d_parts);
        k_vp_sum<<<(unsigned)((nr * n_box + 255) / 256), 256, 0, st>>>(d_parts, n_pairs, n_box, (int)r0,
                                                                      (int)nr, d_sums);
        k_vp_recip<<<dim3((unsigned)n_box, (unsigned)nr), RL_WAVES * 64, lds, st>>>(s.bv, s.recip_order, va,
                                                                                   d_cfac, d_erec);
        oc.launched();
    }
    const VpPart *h_sums = reinterpret_cast<const VpPart *>(oc.stage(d_sums, sm_bytes));
    const double *h_erec = reinterpret_cast<const double *>(oc.stage(d_erec, er_bytes));
    MMC_TRY(oc.finish("mmc_batch_volume_perturb"));

    // the four parts in totals_ewald's arithmetic (energy.jl:978-1021), differences, weights: host, fp64,
    // replica by replica and box by box -- the caller's arrays are written only now
    const double factor = s.bv.factor;
    for (int64_t r = 0; r < R; r++) {
        double u[VP_BOXES][4];
        bool ovl[VP_BOXES];
        for (int k = 0; k < n_box; k++) {
            const VpPart &p = h_sums[(size_t)r * n_box + k];
            u[k][0] = (2.0 * (p.lj * 4)) / 2;          // energy.jl:289, :978-980
            double real = 2.0 * p.qq;
            real *= factor / 2;                         // :1001
            u[k][1] = real;
            u[k][2] = h_erec[(size_t)r * n_box + k] * factor; // :1009
            u[k][3] = -va.kappa[k] * sq2 / sqrt(3.141592653589793) * factor; // ewalds.jl:832
            ovl[k] = p.ovl != 0;
        }
        if (base_out)
            for (int c = 0; c < 4; c++)
                base_out[4 * r + c] = (c == 1 && ovl[0]) ? INFINITY : u[0][c];
        for (int k = 1; k < n_box; k++) {
            double d[4];
            for (int c = 0; c < 4; c++)
                d[c] = u[k][c] - u[0][c];
            const double du = ((d[0] + d[1]) + d[2]) + d[3];
            const bool zero = ovl[0] || ovl[k] || !std::isfinite(du);
            const double sc = scale[k - 1];
            const double w = zero ? 0.0 : exp(-du / temperature + (double)N * log(sc * sc * sc)); // volumeChange.jl:129-130, P = 0
            const size_t o = (size_t)r * n_scale + (k - 1);
            if (boltz_sum)
                boltz_sum[o] += w;
            if (n_overlap)
                n_overlap[o] += zero ? 1 : 0;
            if (du_out)
                for (int c = 0; c < 4; c++)
                    du_out[4 * o + c] = (c == 1 && (ovl[0] || ovl[k])) ? INFINITY : d[c];
        }
    }
    return MMC_OK;
}
