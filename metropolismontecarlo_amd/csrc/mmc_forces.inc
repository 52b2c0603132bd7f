// mmc_forces.inc -- host side of the forces and torques (include/mmc_hip.h, "Forces and torques"; the
// kernels are in mmc_forces.hpp).  Included by mmc_hip.hip after mmc_deletion.inc, whose device
// scratch and pinned staging (mmc_batch::widom_buf, widom_host) the call shares: the calls are
// synchronous and none keeps anything there between calls.
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
    MMC_REQUIRE(!sel || n_sel >= 1, MMC_ERR_ARG, "%s: n_sel must be >= 1", what);
    if (mass)
        for (int a = 0; a < 3; a++)
            MMC_REQUIRE(std::isfinite(mass[a]) && mass[a] > 0.0, MMC_ERR_ARG,
                        "%s: mass[%d] must be positive and finite", what, a);
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

    // ---- device scratch: rows [R n][9] (72 bytes per unit), flags [R n] (1 byte), the atom rows
    // [R n][9] only when atom_out asks for them (72 bytes more), the per-replica block (fsum [R][9],
    // counts [R], S-buffer bits [R] -- one copy each way through the pinned staging of the same
    // layout) and the selection [n] ----
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t nu = (size_t)(R * n);
    const size_t row_bytes = sizeof(double) * FORCES_ROW * nu;
    const size_t sums_bytes = (sizeof(double) * 9 + sizeof(long long)) * (size_t)R, blk_bytes = sums_bytes + (size_t)R;
    const size_t o_flags = up(row_bytes), o_blk = o_flags + up(nu), o_sel = o_blk + up(blk_bytes),
                 o_atom = o_sel + up(sizeof(int32_t) * (size_t)n);
    const size_t bytes = o_atom + (atom_out ? row_bytes : 0);
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
    double *d_rows = reinterpret_cast<double *>(base);
    uint8_t *d_flags = reinterpret_cast<uint8_t *>(base + o_flags);
    double *d_fsum = reinterpret_cast<double *>(base + o_blk);
    long long *d_nflag = reinterpret_cast<long long *>(d_fsum + 9 * R);
    uint8_t *d_scur = reinterpret_cast<uint8_t *>(base + o_blk + sums_bytes);
    int32_t *d_sel = reinterpret_cast<int32_t *>(base + o_sel);
    double *d_atom = atom_out ? reinterpret_cast<double *>(base + o_atom) : nullptr;
    char *hblk = static_cast<char *>(b->widom_host);
    double *h_fsum = reinterpret_cast<double *>(hblk);
    long long *h_nflag = reinterpret_cast<long long *>(h_fsum + 9 * R);
    memset(h_fsum, 0, sizeof(double) * 9 * R);
    for (int64_t r = 0; r < R; r++)
        h_nflag[r] = n_flagged ? (long long)n_flagged[r] : 0;
    memcpy(hblk + sums_bytes, b->s_cur.data(), (size_t)R);
    std::vector<int32_t> h_sel((size_t)n);
    for (int64_t k = 0; k < n; k++)
        h_sel[k] = sel ? sel[k] : (int32_t)k;

    hipStream_t st = s.stream;
    MMC_HIP(hipMemcpyAsync(base + o_blk, hblk, blk_bytes, hipMemcpyHostToDevice, st));
    MMC_HIP(hipMemcpyAsync(d_sel, h_sel.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));

    ForcesArgs fa{};
    fa.sel = d_sel;
    fa.rows = d_rows;
    fa.atom = d_atom;
    fa.flags = d_flags;
    fa.scur = d_scur;
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

    const PairParams pp = mmc_pair_params(b->lj_rcut, b->qq_rcut, 0.0, 0.5, s.bv.kappa, false);
    // the minimum image of an atom pair from its molecules' (IMG): exactly k_move_eval_wave's
    // condition (mmc_batch.inc) -- the molecule is one of the batch's own, bounded by r_mol_max
    const bool img = b->rigid_only && b->image_by_molecule != 0 &&
                     s.image_by_molecule(std::max(pp.lj_gate_sq, pp.qq_gate_sq)) &&
                     s.pairs_inside_slack(pp.qq_gate_sq, pp.qq_slack_sq) &&
                     s.pairs_inside_slack(pp.lj_gate_sq, pp.lj_slack_sq);
    // persistent workgroups as k_move_eval_wave's launches (mmc_batch.inc), capped at option "wave_wgs"
    // or at what is resident: FORCES_OCC waves on each of the 4 SIMDs of every compute unit
    const int64_t n_units = (int64_t)nu;
    int64_t wgs = (n_units + WV_WAVES - 1) / WV_WAVES;
    const int64_t cap = b->wave_wgs > 0 ? b->wave_wgs : (int64_t)(4 * FORCES_OCC / WV_WAVES) * b->n_cus;
    if (wgs > cap) wgs = cap;
    if (img)
        k_forces_wave<true><<<(unsigned)wgs, WV_WAVES * 64, 0, st>>>(s.bv, s.rec, s.qq_tab, s.kpack, s.fc, pp, fa,
                                                                     (int)n_units);
    else
        k_forces_wave<false><<<(unsigned)wgs, WV_WAVES * 64, 0, st>>>(s.bv, s.rec, s.qq_tab, s.kpack, s.fc, pp, fa,
                                                                      (int)n_units);
    MMC_HIP(hipGetLastError());

    ForcesReduceArgs ra{};
    ra.rows = d_rows;
    ra.flags = d_flags;
    ra.fsum = d_fsum;
    ra.n_flag = d_nflag;
    ra.n = (int32_t)n;
    ra.R = (int32_t)R;
    // (a wave per replica; the results do not depend on how many workgroups share the replicas)
    const int64_t rwgs = std::min<int64_t>(R, (int64_t)16 * b->n_cus);
    k_forces_reduce<<<(unsigned)rwgs, 64, 0, st>>>(ra);
    MMC_HIP(hipGetLastError());

    const bool want_rows = force_out || torque_out || vir_out;
    std::vector<double> h_rows(want_rows ? FORCES_ROW * nu : 0), h_atom(atom_out ? 9 * nu : 0);
    if (want_rows)
        MMC_HIP(hipMemcpyAsync(h_rows.data(), d_rows, row_bytes, hipMemcpyDeviceToHost, st));
    if (atom_out)
        MMC_HIP(hipMemcpyAsync(h_atom.data(), d_atom, row_bytes, hipMemcpyDeviceToHost, st));
    MMC_HIP(hipMemcpyAsync(hblk, base + o_blk, sums_bytes, hipMemcpyDeviceToHost, st));
    std::vector<uint8_t> h_flags(ovl_out ? nu : 0);
    if (ovl_out)
        MMC_HIP(hipMemcpyAsync(h_flags.data(), d_flags, nu, hipMemcpyDeviceToHost, st));
    MMC_TRY(s.sync());
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
        memcpy(atom_out, h_atom.data(), row_bytes);
    if (fsum)
        memcpy(fsum, h_fsum, sizeof(double) * 9 * R);
    if (n_flagged)
        for (int64_t r = 0; r < R; r++)
            n_flagged[r] = (int64_t)h_nflag[r];
    if (ovl_out)
        memcpy(ovl_out, h_flags.data(), nu);
    return MMC_OK;
}
