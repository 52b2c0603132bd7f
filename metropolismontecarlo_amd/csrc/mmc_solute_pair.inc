// mmc_solute_pair.inc -- host side of Widom insertion of solute pairs (include/mmc_hip.h, "Solute
// pairs"; the kernels are in mmc_solute_pair.hpp).  Included by mmc_hip.hip after mmc_solute.inc; each
// solute's record, refusals and parameter rows, the state checks, the device scratch, the pinned
// staging, the launch and the drain of the stream are mmc_units.inc's.
#include "mmc_solute_pair.hpp"

static int32_t solute_pair_run(mmc_batch *b, const SoluteIn &A, const SoluteIn &B, const double *eps_ab,
                               const double *sig_ab, int32_t K, const double *d, int64_t M, uint64_t seed, int64_t draw0,
                               const double *mol_a_in, const double *mol_b_in, bool at, double temperature,
                               double *boltz_a, int64_t *n_zero_a, double *boltz_b, int64_t *n_zero_b, double *boltz_ab,
                               int64_t *n_zero_ab, double *mol_a_out, double *mol_b_out, double *du_out,
                               uint8_t *flags_out, const char *what)
{
    // ---- arguments (MMC_ERR_ARG): first what needs no batch, so that it is refused without a device;
    // then state (MMC_ERR_STATE), then scope (MMC_ERR_UNSUPPORTED); nothing is written before every
    // check has passed ----
    MMC_REQUIRE(A.S >= 1 && A.S <= SOL_MAX_SITES - 1, MMC_ERR_ARG, "%s: n_sites_a must be 1..%d", what, SOL_MAX_SITES - 1);
    MMC_REQUIRE(B.S >= 1 && B.S <= SOL_MAX_SITES - 1, MMC_ERR_ARG, "%s: n_sites_b must be 1..%d", what, SOL_MAX_SITES - 1);
    MMC_REQUIRE(A.S + B.S <= SOL_MAX_SITES, MMC_ERR_ARG, "%s: n_sites_a + n_sites_b must be <= %d", what, SOL_MAX_SITES);
    MMC_REQUIRE(K >= 1 && K <= PAIR_MAX_SEP, MMC_ERR_ARG, "%s: n_sep must be 1..%d", what, PAIR_MAX_SEP);
    MMC_TRY(solute_null_args(A, what));
    MMC_TRY(solute_null_args(B, what));
    MMC_REQUIRE(eps_ab, MMC_ERR_ARG, "%s: NULL eps_ab", what);
    MMC_REQUIRE(sig_ab, MMC_ERR_ARG, "%s: NULL sig_ab", what);
    if (at) {
        MMC_REQUIRE(mol_a_in, MMC_ERR_ARG, "%s: NULL mol_a_in", what);
        MMC_REQUIRE(mol_b_in, MMC_ERR_ARG, "%s: NULL mol_b_in", what);
    } else {
        MMC_REQUIRE(A.offsets, MMC_ERR_ARG, "%s: NULL offsets_a", what);
        MMC_REQUIRE(B.offsets, MMC_ERR_ARG, "%s: NULL offsets_b", what);
        MMC_REQUIRE(d, MMC_ERR_ARG, "%s: NULL d", what);
    }
    MMC_REQUIRE(boltz_a && n_zero_a, MMC_ERR_ARG, "%s: boltz_a and n_zero_a are required", what);
    MMC_REQUIRE(boltz_b && n_zero_b, MMC_ERR_ARG, "%s: boltz_b and n_zero_b are required", what);
    MMC_REQUIRE(boltz_ab && n_zero_ab, MMC_ERR_ARG, "%s: boltz_ab and n_zero_ab are required", what);
    MMC_REQUIRE(M >= 1, MMC_ERR_ARG, "%s: n_insert must be >= 1", what);
    MMC_TRY(temperature_arg(temperature, what));
    bool charged = false; // one of the two
    double q2;
    MMC_TRY(solute_value_args(A, what, &charged, &q2));
    MMC_TRY(solute_value_args(B, what, &charged, &q2));
    for (int q = 0; q < A.S * B.S; q++) {
        MMC_REQUIRE(std::isfinite(eps_ab[q]) && eps_ab[q] >= 0.0, MMC_ERR_ARG, "%s: eps_ab must be finite and >= 0", what);
        MMC_REQUIRE(std::isfinite(sig_ab[q]) && sig_ab[q] >= 0.0, MMC_ERR_ARG, "%s: sig_ab must be finite and >= 0", what);
    }
    if (!at)
        for (int k = 0; k < K; k++)
            MMC_REQUIRE(std::isfinite(d[k]) && d[k] > 0.0, MMC_ERR_ARG, "%s: d must be finite and > 0", what);
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    const int64_t R = s.R, nwa = 3 * (int64_t)A.S + 3, nwb = 3 * (int64_t)B.S + 3, nrow = 1 + 2 * (int64_t)K;
    if (!at)
        for (int k = 0; k < K; k++)
            MMC_REQUIRE(d[k] < 0.5 * s.bv.box, MMC_ERR_ARG, "%s: d must be below half the box", what);
    MMC_REQUIRE(R * M * (1 + (int64_t)K) <= (int64_t)INT32_MAX, MMC_ERR_ARG,
                "%s: replicas x n_insert x (1 + n_sep) exceeds 2^31 - 1", what);
    if (at) {
        for (int64_t k = 0; k < R * M * nwa; k++)
            MMC_REQUIRE(std::isfinite(mol_a_in[k]), MMC_ERR_ARG, "%s: non-finite mol_a_in", what);
        for (int64_t k = 0; k < R * M * K * nwb; k++)
            MMC_REQUIRE(std::isfinite(mol_b_in[k]), MMC_ERR_ARG, "%s: non-finite mol_b_in", what);
    }
    MMC_TRY(units_state_scope(b, what));

    // ---- device scratch: terms [R M][1 + 2 K][3], the per-replica block ([R][2 (1 + 2 K)] words:
    // sums, then counts), the flags [R M][1 + K], the solutes' parameters, the A-B table, the
    // separations and the placements ----
    const size_t n = (size_t)(R * M);
    const bool need_a = at || mol_a_out, need_b = at || mol_b_out;
    const int S2 = A.S + B.S;
    UnitsCall uc(b, n, 3 * (int)nrow, 2 * (int)nrow);
    const size_t o_fl = uc.take(n * (1 + K)), o_par = uc.take(sizeof(double) * SOL_PAR * S2),
                 o_x = uc.take(sizeof(double) * 3 * A.S * B.S), o_d = uc.take(sizeof(double) * K),
                 o_ma = uc.take(need_a ? sizeof(double) * nwa * n : 0),
                 o_mb = uc.take(need_b ? sizeof(double) * nwb * K * n : 0);
    MMC_TRY(uc.alloc());
    double *d_par = uc.at<double>(o_par), *d_x = uc.at<double>(o_x), *d_d = uc.at<double>(o_d);
    double *d_ma = need_a ? uc.at<double>(o_ma) : nullptr, *d_mb = need_b ? uc.at<double>(o_mb) : nullptr;
    uint8_t *d_fl = uc.at<uint8_t>(o_fl);
    {   // the staged block: per replica the sums a, b_0 .. b_K-1, ab_0 .. ab_K-1, then the counts alike
        double *w = uc.h_sums();
        for (int64_t r = 0; r < R; r++) {
            double *sm = w + r * 2 * nrow;
            long long *ct = reinterpret_cast<long long *>(sm + nrow);
            sm[0] = boltz_a[r];
            ct[0] = n_zero_a[r];
            for (int k = 0; k < K; k++) {
                sm[1 + k] = boltz_b[r * K + k];
                sm[1 + K + k] = boltz_ab[r * K + k];
                ct[1 + k] = n_zero_b[r * K + k];
                ct[1 + K + k] = n_zero_ab[r * K + k];
            }
        }
    }
    std::vector<double> h_par((size_t)SOL_PAR * S2, 0.0), h_x((size_t)3 * A.S * B.S), h_d((size_t)K, 0.0);
    solute_pack(h_par.data(), A, A.offsets);
    solute_pack(h_par.data() + SOL_PAR * A.S, B, B.offsets);
    for (int q = 0; q < A.S * B.S; q++) {
        h_x[3 * q] = eps_ab[q];
        h_x[3 * q + 1] = sig_ab[q];
        h_x[3 * q + 2] = A.charge[q / B.S] * B.charge[q % B.S];
    }
    if (!at)
        for (int k = 0; k < K; k++)
            h_d[k] = d[k];

    SolutePairArgs sa{};
    sa.seed = seed;
    sa.draw0 = draw0;
    sa.par = d_par;
    sa.xpar = d_x;
    sa.dsep = d_d;
    sa.mol_a_in = at ? d_ma : nullptr;
    sa.mol_b_in = at ? d_mb : nullptr;
    sa.mol_a_out = (!at && mol_a_out) ? d_ma : nullptr;
    sa.mol_b_out = (!at && mol_b_out) ? d_mb : nullptr;
    sa.terms = uc.d_rows();
    sa.flags = d_fl;
    sa.scur = uc.d_scur();
    sa.n_insert = (int32_t)M;
    sa.n_a = A.S;
    sa.n_b = B.S;
    sa.n_sep = K;
    sa.self_a = ewald_self_term(A.charge, A.S, s.bv.kappa, s.bv.factor); // EwaldSelf of each solute
    sa.self_b = ewald_self_term(B.charge, B.S, s.bv.kappa, s.bv.factor);
    const PairParams pp = mmc_pair_params(b->lj_rcut, b->qq_rcut, 0.0, 0.5, s.bv.kappa, false);
    // the instantiation: no reciprocal part and no tables when neither solute carries a charge
    const units_kernel_t<SolutePairArgs> kern = charged ? k_solute_pair_wave<16> : k_solute_pair_wave<0>;
    const int occ = charged ? SOL_OCC(16) : SOL_OCC(0);

    // ---- from here to finish() nothing returns ----
    uc.upload_block();
    uc.to_device(d_par, h_par.data(), sizeof(double) * h_par.size());
    uc.to_device(d_x, h_x.data(), sizeof(double) * h_x.size());
    uc.to_device(d_d, h_d.data(), sizeof(double) * h_d.size());
    if (at) {
        uc.to_device(d_ma, mol_a_in, sizeof(double) * nwa * n);
        uc.to_device(d_mb, mol_b_in, sizeof(double) * nwb * K * n);
    }
    uc.launch(false, kern, kern, occ, pp, sa);
    if (uc.e == hipSuccess)
        k_pair_reduce<<<dim3((unsigned)R, (unsigned)(1 + K)), 64, 0, uc.st>>>(uc.d_rows(), d_fl, (int)M, (int)K,
                                                                              1.0 / temperature, uc.d_sums());
    uc.launched();
    std::vector<double> h_terms, h_ma(mol_a_out ? nwa * n : 0), h_mb(mol_b_out ? nwb * K * n : 0);
    std::vector<uint8_t> h_fl(flags_out ? n * (1 + K) : 0);
    if (mol_a_out)
        uc.to_host(h_ma.data(), d_ma, sizeof(double) * h_ma.size());
    if (mol_b_out)
        uc.to_host(h_mb.data(), d_mb, sizeof(double) * h_mb.size());
    if (flags_out)
        uc.to_host(h_fl.data(), d_fl, h_fl.size());
    MMC_TRY(uc.finish(du_out ? &h_terms : nullptr, nullptr, what));
    // (the caller's arrays are written only once the whole call has succeeded)
    {
        const double *w = uc.h_sums();
        for (int64_t r = 0; r < R; r++) {
            const double *sm = w + r * 2 * nrow;
            const long long *ct = reinterpret_cast<const long long *>(sm + nrow);
            boltz_a[r] = sm[0];
            n_zero_a[r] = ct[0];
            for (int k = 0; k < K; k++) {
                boltz_b[r * K + k] = sm[1 + k];
                boltz_ab[r * K + k] = sm[1 + K + k];
                n_zero_b[r * K + k] = ct[1 + k];
                n_zero_ab[r * K + k] = ct[1 + K + k];
            }
        }
    }
    if (du_out)
        memcpy(du_out, h_terms.data(), sizeof(double) * h_terms.size());
    if (flags_out)
        memcpy(flags_out, h_fl.data(), h_fl.size());
    if (mol_a_out)
        memcpy(mol_a_out, h_ma.data(), sizeof(double) * h_ma.size());
    if (mol_b_out)
        memcpy(mol_b_out, h_mb.data(), sizeof(double) * h_mb.size());
    return MMC_OK;
}

extern "C" int32_t mmc_batch_widom_pair(mmc_batch *b, int32_t n_sites_a, const double *offsets_a, const double *charge_a,
                                        const double *eps_a, const double *sig_a, int32_t n_sites_b,
                                        const double *offsets_b, const double *charge_b, const double *eps_b,
                                        const double *sig_b, const double *eps_ab, const double *sig_ab, int32_t n_sep,
                                        const double *d, int64_t n_insert, uint64_t seed, int64_t draw0,
                                        double temperature, double *boltz_a, int64_t *n_zero_a, double *boltz_b,
                                        int64_t *n_zero_b, double *boltz_ab, int64_t *n_zero_ab, double *mol_a_out,
                                        double *mol_b_out, double *du_out, uint8_t *flags_out)
{
    const SoluteIn A{ n_sites_a, offsets_a, charge_a, eps_a, sig_a, "_a" },
                   B{ n_sites_b, offsets_b, charge_b, eps_b, sig_b, "_b" };
    return solute_pair_run(b, A, B, eps_ab, sig_ab, n_sep, d, n_insert, seed, draw0, nullptr, nullptr, false, temperature,
                           boltz_a, n_zero_a, boltz_b, n_zero_b, boltz_ab, n_zero_ab, mol_a_out, mol_b_out, du_out,
                           flags_out, "mmc_batch_widom_pair");
}

extern "C" int32_t mmc_batch_widom_pair_at(mmc_batch *b, int32_t n_sites_a, const double *charge_a, const double *eps_a,
                                           const double *sig_a, int32_t n_sites_b, const double *charge_b,
                                           const double *eps_b, const double *sig_b, const double *eps_ab,
                                           const double *sig_ab, int32_t n_sep, int64_t n_insert, const double *mol_a_in,
                                           const double *mol_b_in, double temperature, double *boltz_a,
                                           int64_t *n_zero_a, double *boltz_b, int64_t *n_zero_b, double *boltz_ab,
                                           int64_t *n_zero_ab, double *du_out, uint8_t *flags_out)
{
    const SoluteIn A{ n_sites_a, nullptr, charge_a, eps_a, sig_a, "_a" },
                   B{ n_sites_b, nullptr, charge_b, eps_b, sig_b, "_b" };
    return solute_pair_run(b, A, B, eps_ab, sig_ab, n_sep, nullptr, n_insert, 0, 0, mol_a_in, mol_b_in, true, temperature,
                           boltz_a, n_zero_a, boltz_b, n_zero_b, boltz_ab, n_zero_ab, nullptr, nullptr, du_out, flags_out,
                           "mmc_batch_widom_pair_at");
}
