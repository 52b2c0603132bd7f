// mmc_deletion.inc -- host side of the deletion energies (include/mmc_hip.h, "Deletion energies";
// the kernels are in mmc_deletion.hpp).  Included by mmc_hip.hip after mmc_widom.inc, whose device
// scratch and pinned staging (mmc_batch::widom_buf, widom_host) the call shares: both calls are
// synchronous and neither keeps anything there between calls.
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
    MMC_REQUIRE(std::isfinite(temperature) && temperature > 0.0, MMC_ERR_ARG,
                "%s: temperature must be positive and finite", what);
    MMC_REQUIRE(hist || esum || boltz_sum || n_flagged || du_out || ovl_out, MMC_ERR_ARG,
                "%s: every output is NULL", what);
    if (hist) {
        MMC_REQUIRE(n_bins >= 1 && n_bins <= MMC_DELETION_MAX_BINS, MMC_ERR_ARG, "%s: n_bins outside 1..%d", what,
                    MMC_DELETION_MAX_BINS);
        MMC_REQUIRE(std::isfinite(u_lo) && std::isfinite(u_hi) && u_lo < u_hi, MMC_ERR_ARG,
                    "%s: the histogram wants finite u_lo < u_hi", what);
    }
    MMC_REQUIRE(!sel || n_sel >= 1, MMC_ERR_ARG, "%s: n_sel must be >= 1", what);
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    const int64_t R = s.R, N = s.n_mol;
    if (sel)
        for (int32_t k = 0; k < n_sel; k++)
            MMC_REQUIRE(sel[k] >= 0 && sel[k] < N, MMC_ERR_ARG, "%s: sel[%d] = %d outside 0..%lld", what, (int)k,
                        (int)sel[k], (long long)(N - 1));
    const int64_t n = sel ? (int64_t)n_sel : N;
    MMC_REQUIRE(R * n <= (int64_t)INT32_MAX, MMC_ERR_ARG, "%s: replicas x selected molecules exceeds 2^31 - 1", what);
    MMC_REQUIRE(!b->has_prev, MMC_ERR_STATE, "proposals outstanding: call mmc_batch_settle first");
    BATCH_NO_VOLUME_TRIAL(b);
    MMC_REQUIRE(!b->needs_reload, MMC_ERR_STATE, "%s: a run failed half-way; set every replica again", what);
    BATCH_S_FRESH(b, what);
    BATCH_ONE_BOX(b, what);
    BATCH_NOT_WOLF(b, what);
    MMC_REQUIRE(b->fast_ok, MMC_ERR_UNSUPPORTED,
                "%s: needs identical 3-atom molecules and a cutoff / kappa the erfc table covers", what);
    MMC_REQUIRE(N >= 2, MMC_ERR_UNSUPPORTED, "%s: needs at least 2 molecules", what);

    // ---- device scratch: terms [R n][3], flags [R n], the per-replica block (esum [R][4], sums [R],
    // counts [R], S-buffer bits [R] -- one copy each way through the pinned staging of the same
    // layout), the selection [n], the histogram ----
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t nu = (size_t)(R * n);
    const size_t slots = hist ? (size_t)n_bins + 2 : 0, n_hist = slots * (size_t)(per_replica ? R : 1);
    const size_t sums_bytes = (sizeof(double) * 5 + sizeof(long long)) * (size_t)R, blk_bytes = sums_bytes + (size_t)R;
    const size_t o_flags = up(sizeof(double) * 3 * nu), o_blk = o_flags + up(nu), o_sel = o_blk + up(blk_bytes),
                 o_hist = o_sel + up(sizeof(int32_t) * (size_t)n);
    const size_t bytes = o_hist + sizeof(unsigned long long) * n_hist;
    if (bytes > b->widom_bytes) {
        if (b->widom_buf)
            MMC_HIP(hipFree(b->widom_buf));
        b->widom_buf = nullptr;
        b->widom_bytes = 0;
        MMC_HIP(hipMalloc(&b->widom_buf, bytes));
        b->widom_bytes = bytes;
    }
    if (blk_bytes > b->widom_host_bytes) {
        if (b->widom_host)
            MMC_HIP(hipHostFree(b->widom_host));
        b->widom_host = nullptr;
        b->widom_host_bytes = 0;
        MMC_HIP(hipHostMalloc(&b->widom_host, blk_bytes, hipHostMallocDefault));
        b->widom_host_bytes = blk_bytes;
    }
    char *base = static_cast<char *>(b->widom_buf);
    double *d_terms = reinterpret_cast<double *>(base);
    uint8_t *d_flags = reinterpret_cast<uint8_t *>(base + o_flags);
    double *d_esum = reinterpret_cast<double *>(base + o_blk);
    double *d_boltz = d_esum + 4 * R;
    long long *d_nflag = reinterpret_cast<long long *>(d_boltz + R);
    uint8_t *d_scur = reinterpret_cast<uint8_t *>(base + o_blk + sums_bytes);
    int32_t *d_sel = reinterpret_cast<int32_t *>(base + o_sel);
    unsigned long long *d_hist = hist ? reinterpret_cast<unsigned long long *>(base + o_hist) : nullptr;
    char *hblk = static_cast<char *>(b->widom_host);
    double *h_esum = reinterpret_cast<double *>(hblk), *h_boltz = h_esum + 4 * R;
    long long *h_nflag = reinterpret_cast<long long *>(h_boltz + R);
    memset(h_esum, 0, sizeof(double) * 4 * R);
    for (int64_t r = 0; r < R; r++) {
        h_boltz[r] = boltz_sum ? boltz_sum[r] : 0.0;
        h_nflag[r] = n_flagged ? (long long)n_flagged[r] : 0;
    }
    memcpy(hblk + sums_bytes, b->s_cur.data(), (size_t)R);
    std::vector<int32_t> h_sel((size_t)n);
    for (int64_t k = 0; k < n; k++)
        h_sel[k] = sel ? sel[k] : (int32_t)k;

    hipStream_t st = s.stream;
    MMC_HIP(hipMemcpyAsync(base + o_blk, hblk, blk_bytes, hipMemcpyHostToDevice, st));
    MMC_HIP(hipMemcpyAsync(d_sel, h_sel.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
    if (hist)
        MMC_HIP(hipMemsetAsync(d_hist, 0, sizeof(unsigned long long) * n_hist, st));

    DeletionArgs da{};
    da.sel = d_sel;
    da.terms = d_terms;
    da.flags = d_flags;
    da.scur = d_scur;
    da.n = (int32_t)n;
    {   // EwaldSelf(N) - EwaldSelf(N \ i) in orc_ewald_self's arithmetic (ewalds.jl:829-833)
        double q2 = 0.0;
        for (int a = 0; a < 3; a++)
            q2 += s.fc.q[a] * s.fc.q[a];
        da.self_d = -s.bv.kappa * q2 / std::sqrt(M_PI) * s.bv.factor;
    }

    const PairParams pp = mmc_pair_params(b->lj_rcut, b->qq_rcut, 0.0, 0.5, s.bv.kappa, false);
    // the minimum image of an atom pair from its molecules' (WV_IMG): exactly k_move_eval_wave's
    // condition (mmc_batch.inc) -- the molecule is one of the batch's own, bounded by r_mol_max
    const bool img = b->rigid_only && b->image_by_molecule != 0 &&
                     s.image_by_molecule(std::max(pp.lj_gate_sq, pp.qq_gate_sq)) &&
                     s.pairs_inside_slack(pp.qq_gate_sq, pp.qq_slack_sq) &&
                     s.pairs_inside_slack(pp.lj_gate_sq, pp.lj_slack_sq);
    // persistent workgroups as k_move_eval_wave's launches (mmc_batch.inc), capped at option "wave_wgs"
    // or at what is resident: DELETION_OCC waves on each of the 4 SIMDs of every compute unit
    const int64_t n_units = (int64_t)nu;
    int64_t wgs = (n_units + WV_WAVES - 1) / WV_WAVES;
    const int64_t cap = b->wave_wgs > 0 ? b->wave_wgs : (int64_t)(4 * DELETION_OCC / WV_WAVES) * b->n_cus;
    if (wgs > cap) wgs = cap;
    if (img)
        k_deletion_wave<true><<<(unsigned)wgs, WV_WAVES * 64, 0, st>>>(s.bv, s.rec, s.qq_tab, s.kpack, s.fc, pp, da,
                                                                       (int)n_units);
    else
        k_deletion_wave<false><<<(unsigned)wgs, WV_WAVES * 64, 0, st>>>(s.bv, s.rec, s.qq_tab, s.kpack, s.fc, pp, da,
                                                                        (int)n_units);
    MMC_HIP(hipGetLastError());

    DeletionReduceArgs ra{};
    ra.terms = d_terms;
    ra.flags = d_flags;
    ra.esum = d_esum;
    ra.boltz = d_boltz;
    ra.n_flag = d_nflag;
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
    k_deletion_reduce<<<(unsigned)rwgs, 64, lds, st>>>(ra);
    MMC_HIP(hipGetLastError());

    std::vector<double> h_terms(du_out ? 3 * nu : 0);
    if (du_out)
        MMC_HIP(hipMemcpyAsync(h_terms.data(), d_terms, sizeof(double) * 3 * nu, hipMemcpyDeviceToHost, st));
    MMC_HIP(hipMemcpyAsync(hblk, base + o_blk, sums_bytes, hipMemcpyDeviceToHost, st));
    std::vector<uint8_t> h_flags(ovl_out ? nu : 0);
    if (ovl_out)
        MMC_HIP(hipMemcpyAsync(h_flags.data(), d_flags, nu, hipMemcpyDeviceToHost, st));
    std::vector<uint64_t> h_hist(n_hist);
    if (hist)
        MMC_HIP(hipMemcpyAsync(h_hist.data(), d_hist, sizeof(uint64_t) * n_hist, hipMemcpyDeviceToHost, st));
    MMC_TRY(s.sync());
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
