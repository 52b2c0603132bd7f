// mmc_forces.inc -- host side of the forces and torques (include/mmc_hip.h, "Forces and torques"; the
// kernels are in mmc_forces.hpp).  Included by mmc_hip.hip after mmc_units.inc, which holds what the
// call shares with mmc_widom.inc and mmc_deletion.inc: the state checks, the selection, the device
// scratch and pinned staging, the launch and the drain of the stream.
#include "mmc_forces.hpp"

extern "C" int32_t mmc_batch_forces(mmc_batch *b, int32_t n_sel, const int32_t *sel, const double *mass,
                                    double *force_out, double *torque_out, double *vir_out, double *atom_out,
                                    double *fsum, int64_t *n_flagged, uint8_t *ovl_out)
{
    const char *what = "mmc_batch_forces";
    // ---- arguments (MMC_ERR_ARG; those that need no batch first, so that they are refused without a
    // device), then state (MMC_ERR_STATE), then scope (MMC_ERR_UNSUPPORTED); nothing is written
    // before every check has passed ----
    MMC_REQUIRE(force_out || torque_out || vir_out || atom_out || fsum || n_flagged || ovl_out, MMC_ERR_ARG,
                "%s: every output is NULL", what);
    UNITS_SEL_ARG(n_sel, sel, what);
    if (mass)
        for (int a = 0; a < 3; a++)
            MMC_REQUIRE(std::isfinite(mass[a]) && mass[a] > 0.0, MMC_ERR_ARG,
                        "%s: mass[%d] must be positive and finite", what, a);
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    const int64_t R = s.R;
    std::vector<int32_t> h_sel;
    MMC_TRY(units_selection(b, n_sel, sel, what, h_sel));
    MMC_TRY(units_state_scope(b, what));
    MMC_REQUIRE(s.n_mol >= 2, MMC_ERR_UNSUPPORTED, "%s: needs at least 2 molecules", what);

    // ---- device scratch: rows [R n][9] (72 bytes per unit), flags [R n] (1 byte), the per-replica
    // block (fsum [R][9], counts [R]), the selection [n], and the atom rows [R n][9] only when atom_out
    // asks for them (72 bytes more) ----
    const size_t n = h_sel.size(), nu = (size_t)R * n;
    UnitsCall uc(b, nu, FORCES_ROW, 9);
    const size_t o_sel = uc.take(sizeof(int32_t) * n), o_atom = uc.take(atom_out ? uc.row_bytes : 0);
    MMC_TRY(uc.alloc());
    int32_t *d_sel = uc.at<int32_t>(o_sel);
    double *d_atom = atom_out ? uc.at<double>(o_atom) : nullptr;
    double *h_fsum = uc.h_sums();
    long long *h_nflag = uc.h_counts();
    memset(h_fsum, 0, sizeof(double) * 9 * R);
    for (int64_t r = 0; r < R; r++)
        h_nflag[r] = n_flagged ? (long long)n_flagged[r] : 0;

    ForcesArgs fa{};
    fa.sel = d_sel;
    fa.rows = uc.d_rows();
    fa.atom = d_atom;
    fa.flags = uc.d_flags();
    fa.scur = uc.d_scur();
    fa.n = (int32_t)n;
    fa.has_mass = mass ? 1 : 0;
    for (int a = 0; a < 3; a++) {
        fa.mass[a] = mass ? mass[a] : 0.0;
        fa.qrec[a] = (s.bv.factor * (4.0 * M_PI / s.bv.box)) * s.fc.q[a];
    }
    for (int ab = 0; ab < 9; ab++)
        fa.qqf[ab] = s.bv.factor * s.fc.qq9[ab];
    fa.c_exp = 2.0 * s.bv.kappa / std::sqrt(M_PI);
    fa.nk2 = -(s.bv.kappa * s.bv.kappa);

    ForcesReduceArgs ra{};
    ra.rows = uc.d_rows();
    ra.flags = uc.d_flags();
    ra.fsum = uc.d_sums();
    ra.n_flag = uc.d_counts();
    ra.n = (int32_t)n;
    ra.R = (int32_t)R;
    // (a wave per replica; the results do not depend on how many workgroups share the replicas)
    const int64_t rwgs = std::min<int64_t>(R, (int64_t)16 * b->n_cus);

    const PairParams pp = mmc_pair_params(b->lj_rcut, b->qq_rcut, 0.0, 0.5, s.bv.kappa, false);
    const bool img = units_image_by_molecule(b, pp);

    // ---- from here to finish() nothing returns ----
    uc.upload_block();
    uc.to_device(d_sel, h_sel.data(), sizeof(int32_t) * n);
    uc.launch(img, k_forces_wave<true>, k_forces_wave<false>, FORCES_OCC, pp, fa);
    if (uc.e == hipSuccess)
        k_forces_reduce<<<(unsigned)rwgs, 64, 0, uc.st>>>(ra);
    uc.launched();
    const bool want_rows = force_out || torque_out || vir_out;
    std::vector<double> h_rows, h_atom(atom_out ? 9 * nu : 0);
    std::vector<uint8_t> h_flags;
    if (atom_out)
        uc.to_host(h_atom.data(), d_atom, uc.row_bytes);
    MMC_TRY(uc.finish(want_rows ? &h_rows : nullptr, ovl_out ? &h_flags : nullptr, what));
    // (the caller's arrays are written only once the whole call has succeeded)
    for (size_t u = 0; want_rows && u < nu; u++) {
        const double *o = h_rows.data() + FORCES_ROW * u;
        for (int k = 0; k < 3; k++) {
            if (force_out)
                force_out[3 * u + k] = o[k];
            if (torque_out)
                torque_out[3 * u + k] = o[3 + k];
            if (vir_out)
                vir_out[3 * u + k] = o[6 + k];
        }
    }
    if (atom_out)
        memcpy(atom_out, h_atom.data(), uc.row_bytes);
    if (fsum)
        memcpy(fsum, h_fsum, sizeof(double) * 9 * R);
    if (n_flagged)
        for (int64_t r = 0; r < R; r++)
            n_flagged[r] = (int64_t)h_nflag[r];
    if (ovl_out)
        memcpy(ovl_out, h_flags.data(), nu);
    return MMC_OK;
}
