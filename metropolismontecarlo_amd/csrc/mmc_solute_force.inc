// mmc_solute_force.inc -- host side of mmc_batch_solute_forces (include/mmc_hip.h, "A fixed solute"; the
// kernels are in mmc_solute_force.hpp): the checks, one ObsCall with the phase table of the call and the
// outputs that were asked for, two launches.  Included by mmc_hip.hip after mmc_solute_chain.inc.
#include "mmc_solute_force.hpp"

extern "C" int32_t mmc_batch_solute_forces(mmc_batch *b, double *force_out, double *torque_out, double *site_lj_out,
                                           double *field_out, double *phi_out, double *recip_out, uint8_t *flags_out)
{
    const char *what = "mmc_batch_solute_forces";
    MMC_REQUIRE(force_out || torque_out || site_lj_out || field_out || phi_out || recip_out || flags_out, MMC_ERR_ARG,
                "%s: every output is NULL", what);
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    STRUCT_STATE(b);
    MMC_REQUIRE(b->sol.n > 0, MMC_ERR_STATE, "%s: no solute is set (mmc_batch_set_solute)", what);
    MMC_REQUIRE(!b->needs_reload, MMC_ERR_STATE, "%s: a run failed half-way; set every replica again", what);
    BATCH_S_FRESH(b, what);
    // (one box, Ewald style, fast_ok and the records in step: mmc_batch_set_solute fences the rest)
    MMC_REQUIRE(struct_use_rec(b), MMC_ERR_UNSUPPORTED, "%s: the batch does not keep its molecules' records in step", what);

    const size_t R = (size_t)s.R, S = (size_t)b->sol.n, nkv = (size_t)s.bv.nkvecs;
    const bool want_ft = force_out || torque_out;
    ObsCall oc(b);
    const size_t o_etab = oc.take(sizeof(cplx) * S * nkv), o_scur = oc.take(R);
    const size_t o_ft = oc.take(want_ft ? sizeof(double) * 6 * R : 0);
    const size_t o_lj = oc.take(site_lj_out ? sizeof(double) * 3 * S * R : 0);
    const size_t o_field = oc.take(field_out ? sizeof(double) * 3 * S * R : 0);
    const size_t o_phi = oc.take(phi_out ? sizeof(double) * S * R : 0);
    const size_t o_recip = oc.take(recip_out ? sizeof(double) * 4 * S * R : 0);
    const size_t o_flags = oc.take(flags_out ? R : 0);
    MMC_TRY(oc.alloc());

    SoluteForceArgs fa{};
    fa.etab = oc.at<cplx>(o_etab);
    fa.scur = oc.at<uint8_t>(o_scur);
    fa.ft = want_ft ? oc.at<double>(o_ft) : nullptr;
    fa.site_lj = site_lj_out ? oc.at<double>(o_lj) : nullptr;
    fa.field = field_out ? oc.at<double>(o_field) : nullptr;
    fa.phi = phi_out ? oc.at<double>(o_phi) : nullptr;
    fa.recip = recip_out ? oc.at<double>(o_recip) : nullptr;
    fa.flags = flags_out ? oc.at<uint8_t>(o_flags) : nullptr;
    for (int a = 0; a < 3; a++) {
        fa.qw[a] = s.fc.q[a];
        fa.fq[a] = s.bv.factor * s.fc.q[a];
    }
    fa.c_exp = 2.0 * s.bv.kappa / std::sqrt(M_PI);
    fa.nk2 = -(s.bv.kappa * s.bv.kappa);
    fa.f_rec = s.bv.factor * (4.0 * M_PI / s.bv.box);
    fa.f_phi = 2.0 * s.bv.factor;
    fa.c_self = 2.0 * s.bv.factor * s.bv.kappa / std::sqrt(M_PI);
    fa.R = (int32_t)R;
    const PairParams pp = mmc_pair_params(b->lj_rcut, b->qq_rcut, 0.0, 0.5, s.bv.kappa, false);

    // ---- from here to finish() nothing returns ----
    oc.to_device(oc.at<uint8_t>(o_scur), b->s_cur.data(), R);
    if (oc.e == hipSuccess) {
        k_solute_phase<<<1, MMC_BLOCK, 0, oc.st>>>(s.bv, b->sol.view(), oc.at<cplx>(o_etab));
        k_solute_force<<<solute_grid(b), SOLC_WAVES * 64, 0, oc.st>>>(s.bv, s.rec, b->sol.view(), s.qq_tab, pp, fa);
    }
    oc.launched();
    const double *h_ft = want_ft ? reinterpret_cast<const double *>(oc.stage(fa.ft, sizeof(double) * 6 * R)) : nullptr;
    oc.fetch(site_lj_out, fa.site_lj, sizeof(double) * 3 * S * R);
    oc.fetch(field_out, fa.field, sizeof(double) * 3 * S * R);
    oc.fetch(phi_out, fa.phi, sizeof(double) * S * R);
    oc.fetch(recip_out, fa.recip, sizeof(double) * 4 * S * R);
    oc.fetch(flags_out, fa.flags, R);
    MMC_TRY(oc.finish(what)); // (the caller's arrays are written only once the whole call has succeeded)
    for (size_t r = 0; want_ft && r < R; r++)
        for (int d = 0; d < 3; d++) {
            if (force_out)
                force_out[3 * r + d] = h_ft[6 * r + d];
            if (torque_out)
                torque_out[3 * r + d] = h_ft[6 * r + 3 + d];
        }
    return MMC_OK;
}
