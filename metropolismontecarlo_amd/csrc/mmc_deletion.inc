// mmc_deletion.inc -- host side of the deletion energies (include/mmc_hip.h, "Deletion energies";
// the kernels are in mmc_deletion.hpp).  Included by mmc_hip.hip after mmc_units.inc, which holds what
// the call shares with mmc_widom.inc and mmc_forces.inc: the state checks, the selection, the device
// scratch and pinned staging, the launch and the drain of the stream.
#include "mmc_deletion.hpp"

#define MMC_DELETION_MAX_BINS 4096

extern "C" int32_t mmc_batch_deletion(mmc_batch *b, int32_t n_sel, const int32_t *sel, double temperature,
                                      int32_t n_bins, double u_lo, double u_hi, int32_t per_replica,
                                      uint64_t *hist, double *esum, double *boltz_sum, int64_t *n_flagged,
                                      double *du_out, uint8_t *ovl_out)
{
    const char *what = "mmc_batch_deletion";
    // ---- arguments (MMC_ERR_ARG; those that need no batch first, so that they are refused without a
    // device), then state (MMC_ERR_STATE), then scope (MMC_ERR_UNSUPPORTED); nothing is written
    // before every check has passed ----
    MMC_TRY(temperature_arg(temperature, what));
    MMC_REQUIRE(hist || esum || boltz_sum || n_flagged || du_out || ovl_out, MMC_ERR_ARG,
                "%s: every output is NULL", what);
    if (hist) {
        MMC_REQUIRE(n_bins >= 1 && n_bins <= MMC_DELETION_MAX_BINS, MMC_ERR_ARG, "%s: n_bins outside 1..%d", what,
                    MMC_DELETION_MAX_BINS);
        MMC_REQUIRE(std::isfinite(u_lo) && std::isfinite(u_hi) && u_lo < u_hi, MMC_ERR_ARG,
                    "%s: the histogram wants finite u_lo < u_hi", what);
    }
    UNITS_SEL_ARG(n_sel, sel, what);
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    const int64_t R = s.R;
    std::vector<int32_t> h_sel;
    MMC_TRY(units_selection(b, n_sel, sel, what, h_sel));
    MMC_TRY(units_state_scope(b, what));
    MMC_REQUIRE(s.n_mol >= 2, MMC_ERR_UNSUPPORTED, "%s: needs at least 2 molecules", what);

    // ---- device scratch: terms [R n][3], flags [R n], the per-replica block (esum [R][4], sums [R],
    // counts [R]), the selection [n], the histogram ----
    const size_t n = h_sel.size(), nu = (size_t)R * n;
    const size_t slots = hist ? (size_t)n_bins + 2 : 0, n_hist = slots * (size_t)(per_replica ? R : 1);
    UnitsCall uc(b, nu, 3, 5);
    const size_t o_sel = uc.take(sizeof(int32_t) * n), o_hist = uc.take(sizeof(unsigned long long) * n_hist);
    MMC_TRY(uc.alloc());
    int32_t *d_sel = uc.at<int32_t>(o_sel);
    unsigned long long *d_hist = hist ? uc.at<unsigned long long>(o_hist) : nullptr;
    double *h_esum = uc.h_sums(), *h_boltz = h_esum + 4 * R;
    long long *h_nflag = uc.h_counts();
    memset(h_esum, 0, sizeof(double) * 4 * R);
    for (int64_t r = 0; r < R; r++) {
        h_boltz[r] = boltz_sum ? boltz_sum[r] : 0.0;
        h_nflag[r] = n_flagged ? (long long)n_flagged[r] : 0;
    }

    DeletionArgs da{};
    da.sel = d_sel;
    da.terms = uc.d_rows();
    da.flags = uc.d_flags();
    da.scur = uc.d_scur();
    da.n = (int32_t)n;
    da.self_d = ewald_self_term(s.fc.q, 3, s.bv.kappa, s.bv.factor); // EwaldSelf(N) - EwaldSelf(N \ i)

    DeletionReduceArgs ra{};
    ra.terms = uc.d_rows();
    ra.flags = uc.d_flags();
    ra.esum = uc.d_sums();
    ra.boltz = uc.d_sums() + 4 * R;
    ra.n_flag = uc.d_counts();
    ra.hist = d_hist;
    ra.u_lo = u_lo;
    ra.u_hi = u_hi;
    ra.scale = hist ? (double)n_bins / (u_hi - u_lo) : 0.0;
    ra.inv_temp = 1.0 / temperature;
    ra.n = (int32_t)n;
    ra.n_bins = hist ? n_bins : 0;
    ra.per_replica = per_replica ? 1 : 0;
    ra.R = (int32_t)R;
    // (a wave per replica; the results do not depend on how many workgroups share the replicas)
    const int64_t rwgs = std::min<int64_t>(R, (int64_t)16 * b->n_cus);
    const size_t lds = (hist && !per_replica) ? sizeof(unsigned int) * slots : 0;

    const PairParams pp = mmc_pair_params(b->lj_rcut, b->qq_rcut, 0.0, 0.5, s.bv.kappa, false);
    const bool img = units_image_by_molecule(b, pp);

    // ---- from here to finish() nothing returns ----
    uc.upload_block();
    uc.to_device(d_sel, h_sel.data(), sizeof(int32_t) * n);
    if (hist && uc.e == hipSuccess)
        uc.e = hipMemsetAsync(d_hist, 0, sizeof(unsigned long long) * n_hist, uc.st);
    uc.launch(img, k_deletion_wave<true>, k_deletion_wave<false>, DELETION_OCC, pp, da);
    if (uc.e == hipSuccess)
        k_deletion_reduce<<<(unsigned)rwgs, 64, lds, uc.st>>>(ra);
    uc.launched();
    std::vector<double> h_terms;
    std::vector<uint8_t> h_flags;
    std::vector<uint64_t> h_hist(n_hist);
    if (hist)
        uc.to_host(h_hist.data(), d_hist, sizeof(uint64_t) * n_hist);
    MMC_TRY(uc.finish(du_out ? &h_terms : nullptr, ovl_out ? &h_flags : nullptr, what));
    // (the caller's arrays are written only once the whole call has succeeded)
    if (hist)
        memcpy(hist, h_hist.data(), sizeof(uint64_t) * n_hist);
    if (esum)
        memcpy(esum, h_esum, sizeof(double) * 4 * R);
    if (boltz_sum)
        memcpy(boltz_sum, h_boltz, sizeof(double) * R);
    if (n_flagged)
        for (int64_t r = 0; r < R; r++)
            n_flagged[r] = (int64_t)h_nflag[r];
    if (du_out)
        memcpy(du_out, h_terms.data(), sizeof(double) * 3 * nu);
    if (ovl_out)
        memcpy(ovl_out, h_flags.data(), nu);
    return MMC_OK;
}
