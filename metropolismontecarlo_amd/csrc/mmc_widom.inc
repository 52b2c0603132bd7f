// mmc_widom.inc -- host side of Widom test-particle insertion (include/mmc_hip.h, "Widom
// test-particle insertion"; the kernels are in mmc_widom.hpp).  Included by mmc_hip.hip after
// mmc_batch.inc.
#include "mmc_widom.hpp"

// Largest distance of an atom from its COM over the caller's molecules [n][12] (atoms, COM), or
// +inf when a COM lies outside [0, L] (the per-molecule image is then not taken).
static double widom_extent(const double *mol, int64_t n, double box)
{
    double m2 = 0.0;
    for (int64_t i = 0; i < n; i++) {
        const double *m = mol + 12 * i;
        for (int d = 0; d < 3; d++)
            if (!(m[9 + d] >= 0.0 && m[9 + d] <= box))
                return INFINITY;
        for (int a = 0; a < 3; a++) {
            const double dx = m[3 * a] - m[9], dy = m[3 * a + 1] - m[10], dz = m[3 * a + 2] - m[11];
            m2 = std::max(m2, dx * dx + dy * dy + dz * dz);
        }
    }
    return std::sqrt(m2);
}

static int32_t widom_run(mmc_batch *b, int64_t M, uint64_t seed, int64_t draw0, const double *offsets,
                         const double *mol_in, double temperature, double *boltz_sum, int64_t *n_overlap,
                         double *mol_out, double *du_out, uint8_t *ovl_out, const char *what)
{
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    const int64_t R = s.R;
    // ---- arguments (MMC_ERR_ARG), then state (MMC_ERR_STATE), then scope (MMC_ERR_UNSUPPORTED);
    // nothing is written before every check has passed ----
    MMC_REQUIRE(M >= 1, MMC_ERR_ARG, "%s: n_insert must be >= 1", what);
    MMC_REQUIRE(R * M <= (int64_t)INT32_MAX, MMC_ERR_ARG, "%s: replicas x n_insert exceeds 2^31 - 1", what);
    MMC_REQUIRE(boltz_sum && n_overlap, MMC_ERR_ARG, "%s: boltz_sum and n_overlap are required", what);
    MMC_REQUIRE(offsets || mol_in, MMC_ERR_ARG, "%s: NULL %s", what, mol_in ? "mol_in" : "offsets");
    MMC_REQUIRE(std::isfinite(temperature) && temperature > 0.0, MMC_ERR_ARG,
                "%s: temperature must be positive and finite", what);
    double r_test = 0.0; // the test molecule's extent about its COM
    if (offsets) {
        for (int q = 0; q < 9; q++)
            MMC_REQUIRE(std::isfinite(offsets[q]), MMC_ERR_ARG, "%s: non-finite offsets", what);
        for (int a = 0; a < 3; a++)
            r_test = std::max(r_test, std::sqrt(offsets[3 * a] * offsets[3 * a] + offsets[3 * a + 1] * offsets[3 * a + 1]
                                                + offsets[3 * a + 2] * offsets[3 * a + 2]));
    } else {
        for (int64_t k = 0; k < R * M * 12; k++)
            MMC_REQUIRE(std::isfinite(mol_in[k]), MMC_ERR_ARG, "%s: non-finite mol_in", what);
        r_test = widom_extent(mol_in, R * M, s.box);
    }
    MMC_REQUIRE(!b->has_prev, MMC_ERR_STATE, "proposals outstanding: call mmc_batch_settle first");
    BATCH_NO_VOLUME_TRIAL(b);
    MMC_REQUIRE(!b->needs_reload, MMC_ERR_STATE, "%s: a run failed half-way; set every replica again", what);
    BATCH_S_FRESH(b, what);
    BATCH_ONE_BOX(b, what);
    BATCH_NOT_WOLF(b, what);
    MMC_REQUIRE(b->fast_ok, MMC_ERR_UNSUPPORTED,
                "%s: needs identical 3-atom molecules and a cutoff / kappa the erfc table covers", what);

    // ---- device scratch: terms [R M][4], flags [R M], the per-replica block (sums [R], counts [R],
    // S-buffer bits [R] -- one copy each way through the pinned staging of the same layout),
    // offsets [9], molecules [R M][12] ----
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t n = (size_t)(R * M);
    const size_t sums_bytes = (sizeof(double) + sizeof(long long)) * (size_t)R, blk_bytes = sums_bytes + (size_t)R;
    const size_t o_flags = up(sizeof(double) * 4 * n), o_blk = o_flags + up(n), o_off = o_blk + up(blk_bytes),
                 o_mol = o_off + up(sizeof(double) * 9);
    const bool need_mol = mol_in || mol_out;
    const size_t bytes = o_mol + (need_mol ? sizeof(double) * 12 * n : 0);
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
    double *d_boltz = reinterpret_cast<double *>(base + o_blk);
    long long *d_novl = reinterpret_cast<long long *>(base + o_blk + sizeof(double) * R);
    uint8_t *d_scur = reinterpret_cast<uint8_t *>(base + o_blk + sums_bytes);
    double *d_off = reinterpret_cast<double *>(base + o_off);
    double *d_mol = need_mol ? reinterpret_cast<double *>(base + o_mol) : nullptr;
    char *hblk = static_cast<char *>(b->widom_host);
    memcpy(hblk, boltz_sum, sizeof(double) * R);
    memcpy(hblk + sizeof(double) * R, n_overlap, sizeof(long long) * R);
    memcpy(hblk + sums_bytes, b->s_cur.data(), (size_t)R);

    hipStream_t st = s.stream;
    MMC_HIP(hipMemcpyAsync(base + o_blk, hblk, blk_bytes, hipMemcpyHostToDevice, st));
    if (offsets)
        MMC_HIP(hipMemcpyAsync(d_off, offsets, sizeof(double) * 9, hipMemcpyHostToDevice, st));
    if (mol_in)
        MMC_HIP(hipMemcpyAsync(d_mol, mol_in, sizeof(double) * 12 * n, hipMemcpyHostToDevice, st));

    WidomArgs wa{};
    wa.seed = seed;
    wa.draw0 = draw0;
    wa.off = d_off;
    wa.mol_in = mol_in ? d_mol : nullptr;
    wa.mol_out = (!mol_in && mol_out) ? d_mol : nullptr;
    wa.terms = d_terms;
    wa.flags = d_flags;
    wa.scur = d_scur;
    wa.n_insert = (int32_t)M;
    {   // EwaldSelf(N+1) - EwaldSelf(N) in orc_ewald_self's arithmetic (ewalds.jl:829-833)
        double q2 = 0.0;
        for (int a = 0; a < 3; a++)
            q2 += s.fc.q[a] * s.fc.q[a];
        wa.self_d = -s.bv.kappa * q2 / std::sqrt(M_PI) * s.bv.factor;
    }

    const PairParams pp = mmc_pair_params(b->lj_rcut, b->qq_rcut, 0.0, 0.5, s.bv.kappa, false);
    // the minimum image of an atom pair from its molecules' (WV_IMG): k_move_eval_wave's condition,
    // gate + r_mol + r_test < box / 2 and inside the slack of the pair tests, where the chains'
    // molecules are known to be rigid
    const double far = std::sqrt(std::max(pp.lj_gate_sq, pp.qq_gate_sq)) + s.r_mol_max + r_test + 1e-6;
    const bool img = b->rigid_only && b->image_by_molecule != 0 && std::isfinite(far) && far < 0.5 * s.box &&
                     far * far < pp.qq_slack_sq && far * far < pp.lj_slack_sq;
    // persistent workgroups as k_move_eval_wave's launches (mmc_batch.inc), capped at option "wave_wgs"
    // or at what is resident: WIDOM_OCC waves on each of the 4 SIMDs of every compute unit
    const int64_t n_units = (int64_t)n;
    int64_t wgs = (n_units + WV_WAVES - 1) / WV_WAVES;
    const int64_t cap = b->wave_wgs > 0 ? b->wave_wgs : (int64_t)(4 * WIDOM_OCC / WV_WAVES) * b->n_cus;
    if (wgs > cap) wgs = cap;
    if (img)
        k_widom_wave<true><<<(unsigned)wgs, WV_WAVES * 64, 0, st>>>(s.bv, s.rec, s.qq_tab, s.kpack, s.fc, pp, wa,
                                                                    (int)n_units);
    else
        k_widom_wave<false><<<(unsigned)wgs, WV_WAVES * 64, 0, st>>>(s.bv, s.rec, s.qq_tab, s.kpack, s.fc, pp, wa,
                                                                     (int)n_units);
    MMC_HIP(hipGetLastError());
    k_widom_reduce<<<(unsigned)R, 64, 0, st>>>(d_terms, d_flags, (int)M, 1.0 / temperature, d_boltz, d_novl);
    MMC_HIP(hipGetLastError());

    std::vector<double> h_terms(du_out ? 4 * n : 0);
    if (du_out)
        MMC_HIP(hipMemcpyAsync(h_terms.data(), d_terms, sizeof(double) * 4 * n, hipMemcpyDeviceToHost, st));
    MMC_HIP(hipMemcpyAsync(hblk, base + o_blk, sums_bytes, hipMemcpyDeviceToHost, st));
    std::vector<uint8_t> h_flags(ovl_out ? n : 0);
    if (ovl_out)
        MMC_HIP(hipMemcpyAsync(h_flags.data(), d_flags, n, hipMemcpyDeviceToHost, st));
    std::vector<double> h_mol(mol_out ? 12 * n : 0);
    if (mol_out)
        MMC_HIP(hipMemcpyAsync(h_mol.data(), d_mol, sizeof(double) * 12 * n, hipMemcpyDeviceToHost, st));
    MMC_TRY(s.sync());
    // (the caller's arrays are written only once the whole call has succeeded)
    memcpy(boltz_sum, hblk, sizeof(double) * R);
    memcpy(n_overlap, hblk + sizeof(double) * R, sizeof(long long) * R);
    if (du_out)
        for (size_t i = 0; i < n; i++)
            for (int c = 0; c < 3; c++)
                du_out[3 * i + c] = h_terms[4 * i + c];
    if (ovl_out)
        memcpy(ovl_out, h_flags.data(), n);
    if (mol_out)
        memcpy(mol_out, h_mol.data(), sizeof(double) * 12 * n);
    return MMC_OK;
}

extern "C" int32_t mmc_batch_widom(mmc_batch *b, int64_t n_insert, uint64_t seed, int64_t draw0,
                                   const double *offsets, double temperature, double *boltz_sum,
                                   int64_t *n_overlap, double *mol_out, double *du_out, uint8_t *ovl_out)
{
    MMC_REQUIRE(offsets, MMC_ERR_ARG, "mmc_batch_widom: NULL offsets");
    return widom_run(b, n_insert, seed, draw0, offsets, nullptr, temperature, boltz_sum, n_overlap, mol_out,
                     du_out, ovl_out, "mmc_batch_widom");
}

extern "C" int32_t mmc_batch_widom_at(mmc_batch *b, int64_t n_insert, const double *mol_in, double temperature,
                                      double *boltz_sum, int64_t *n_overlap, double *du_out, uint8_t *ovl_out)
{
    MMC_REQUIRE(mol_in, MMC_ERR_ARG, "mmc_batch_widom_at: NULL mol_in");
    return widom_run(b, n_insert, 0, 0, nullptr, mol_in, temperature, boltz_sum, n_overlap, nullptr, du_out,
                     ovl_out, "mmc_batch_widom_at");
}
