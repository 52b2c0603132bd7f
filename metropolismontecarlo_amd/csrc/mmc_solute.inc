// mmc_solute.inc -- host side of Widom insertion of foreign rigid solutes (include/mmc_hip.h,
// "Foreign solutes"; the kernel is in mmc_solute.hpp, the reduce kernel is mmc_widom.hpp's).
// Included by mmc_hip.hip after mmc_widom.inc; the state checks, the device scratch, the pinned
// staging, the launch and the drain of the stream are mmc_units.inc's.
#include "mmc_solute.hpp"

static int32_t solute_run(mmc_batch *b, int32_t S, const double *offsets, const double *charge, const double *eps,
                          const double *sig, int64_t M, uint64_t seed, int64_t draw0, const double *mol_in, bool at,
                          double temperature, double *boltz_sum, int64_t *n_overlap, double *mol_out, double *du_out,
                          uint8_t *ovl_out, const char *what)
{
    // ---- arguments (MMC_ERR_ARG): first what needs no batch, so that it is refused without a device;
    // then state (MMC_ERR_STATE), then scope (MMC_ERR_UNSUPPORTED); nothing is written before every
    // check has passed ----
    MMC_REQUIRE(S >= 1 && S <= SOL_MAX_SITES, MMC_ERR_ARG, "%s: n_sites must be 1..%d", what, SOL_MAX_SITES);
    MMC_REQUIRE(charge, MMC_ERR_ARG, "%s: NULL charge", what);
    MMC_REQUIRE(eps, MMC_ERR_ARG, "%s: NULL eps", what);
    MMC_REQUIRE(sig, MMC_ERR_ARG, "%s: NULL sig", what);
    if (at)
        MMC_REQUIRE(mol_in, MMC_ERR_ARG, "%s: NULL mol_in", what);
    else
        MMC_REQUIRE(offsets, MMC_ERR_ARG, "%s: NULL offsets", what);
    MMC_REQUIRE(boltz_sum && n_overlap, MMC_ERR_ARG, "%s: boltz_sum and n_overlap are required", what);
    MMC_REQUIRE(M >= 1, MMC_ERR_ARG, "%s: n_insert must be >= 1", what);
    MMC_REQUIRE(std::isfinite(temperature) && temperature > 0.0, MMC_ERR_ARG,
                "%s: temperature must be positive and finite", what);
    bool charged = false;
    for (int a = 0; a < S; a++) {
        MMC_REQUIRE(std::isfinite(charge[a]), MMC_ERR_ARG, "%s: non-finite charge", what);
        charged = charged || charge[a] != 0.0;
    }
    for (int q = 0; q < 3 * S; q++) {
        MMC_REQUIRE(std::isfinite(eps[q]) && eps[q] >= 0.0, MMC_ERR_ARG, "%s: eps must be finite and >= 0", what);
        MMC_REQUIRE(std::isfinite(sig[q]) && sig[q] >= 0.0, MMC_ERR_ARG, "%s: sig must be finite and >= 0", what);
        if (!at)
            MMC_REQUIRE(std::isfinite(offsets[q]), MMC_ERR_ARG, "%s: non-finite offsets", what);
    }
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    const int64_t R = s.R, nw = 3 * (int64_t)S + 3;
    MMC_REQUIRE(R * M <= (int64_t)INT32_MAX, MMC_ERR_ARG, "%s: replicas x n_insert exceeds 2^31 - 1", what);
    if (at)
        for (int64_t k = 0; k < R * M * nw; k++)
            MMC_REQUIRE(std::isfinite(mol_in[k]), MMC_ERR_ARG, "%s: non-finite mol_in", what);
    MMC_TRY(units_state_scope(b, what));

    // ---- device scratch: terms [R M][4], flags [R M], the per-replica block (sums [R], counts [R]),
    // the solute [S][SOL_PAR], the solutes' sites [R M][S + 1][3] ----
    const size_t n = (size_t)(R * M);
    const bool need_mol = at || mol_out;
    UnitsCall uc(b, n, 4, 1);
    const size_t o_par = uc.take(sizeof(double) * SOL_PAR * S),
                 o_mol = uc.take(need_mol ? sizeof(double) * nw * n : 0);
    MMC_TRY(uc.alloc());
    double *d_par = uc.at<double>(o_par), *d_mol = need_mol ? uc.at<double>(o_mol) : nullptr;
    memcpy(uc.h_sums(), boltz_sum, sizeof(double) * R);
    memcpy(uc.h_counts(), n_overlap, sizeof(long long) * R);
    std::vector<double> h_par((size_t)SOL_PAR * S, 0.0);
    for (int a = 0; a < S; a++) {
        double *p = h_par.data() + SOL_PAR * a;
        for (int d = 0; d < 3; d++) {
            p[d] = at ? 0.0 : offsets[3 * a + d];
            p[4 + d] = eps[3 * a + d];
            p[7 + d] = sig[3 * a + d];
        }
        p[3] = charge[a];
    }

    SoluteArgs sa{};
    sa.seed = seed;
    sa.draw0 = draw0;
    sa.par = d_par;
    sa.mol_in = at ? d_mol : nullptr;
    sa.mol_out = (!at && mol_out) ? d_mol : nullptr;
    sa.terms = uc.d_rows();
    sa.flags = uc.d_flags();
    sa.scur = uc.d_scur();
    sa.n_insert = (int32_t)M;
    sa.n_sites = S;
    {   // EwaldSelf(N+1) - EwaldSelf(N) in orc_ewald_self's arithmetic (ewalds.jl:829-833)
        double q2 = 0.0;
        for (int a = 0; a < S; a++)
            q2 += charge[a] * charge[a];
        sa.self_d = -s.bv.kappa * q2 / std::sqrt(M_PI) * s.bv.factor;
    }
    const PairParams pp = mmc_pair_params(b->lj_rcut, b->qq_rcut, 0.0, 0.5, s.bv.kappa, false);
    // the instantiation: no reciprocal part for an uncharged solute, else the smallest phase tables
    const units_kernel_t<SoluteArgs> kern = !charged ? k_solute_wave<0> : S <= 4 ? k_solute_wave<4> : k_solute_wave<16>;
    const int occ = !charged ? SOL_OCC(0) : S <= 4 ? SOL_OCC(4) : SOL_OCC(16);

    // ---- from here to finish() nothing returns ----
    uc.upload_block();
    uc.to_device(d_par, h_par.data(), sizeof(double) * h_par.size());
    if (at)
        uc.to_device(d_mol, mol_in, sizeof(double) * nw * n);
    uc.launch(false, kern, kern, occ, pp, sa);
    if (uc.e == hipSuccess)
        k_widom_reduce<<<(unsigned)R, 64, 0, uc.st>>>(uc.d_rows(), uc.d_flags(), (int)M, 1.0 / temperature, uc.d_sums(),
                                                     uc.d_counts());
    uc.launched();
    std::vector<double> h_terms, h_mol(mol_out ? nw * n : 0);
    std::vector<uint8_t> h_flags;
    if (mol_out)
        uc.to_host(h_mol.data(), d_mol, sizeof(double) * nw * n);
    MMC_TRY(uc.finish(du_out ? &h_terms : nullptr, ovl_out ? &h_flags : nullptr, what));
    // (the caller's arrays are written only once the whole call has succeeded)
    memcpy(boltz_sum, uc.h_sums(), sizeof(double) * R);
    memcpy(n_overlap, uc.h_counts(), sizeof(long long) * R);
    if (du_out)
        for (size_t i = 0; i < n; i++)
            for (int c = 0; c < 3; c++)
                du_out[3 * i + c] = h_terms[4 * i + c];
    if (ovl_out)
        memcpy(ovl_out, h_flags.data(), n);
    if (mol_out)
        memcpy(mol_out, h_mol.data(), sizeof(double) * nw * n);
    return MMC_OK;
}

extern "C" int32_t mmc_batch_widom_solute(mmc_batch *b, int32_t n_sites, const double *offsets, const double *charge,
                                          const double *eps, const double *sig, int64_t n_insert, uint64_t seed,
                                          int64_t draw0, double temperature, double *boltz_sum, int64_t *n_overlap,
                                          double *mol_out, double *du_out, uint8_t *ovl_out)
{
    return solute_run(b, n_sites, offsets, charge, eps, sig, n_insert, seed, draw0, nullptr, false, temperature,
                      boltz_sum, n_overlap, mol_out, du_out, ovl_out, "mmc_batch_widom_solute");
}

extern "C" int32_t mmc_batch_widom_solute_at(mmc_batch *b, int32_t n_sites, const double *charge, const double *eps,
                                             const double *sig, int64_t n_insert, const double *mol_in,
                                             double temperature, double *boltz_sum, int64_t *n_overlap,
                                             double *du_out, uint8_t *ovl_out)
{
    return solute_run(b, n_sites, nullptr, charge, eps, sig, n_insert, 0, 0, mol_in, true, temperature, boltz_sum,
                      n_overlap, nullptr, du_out, ovl_out, "mmc_batch_widom_solute_at");
}
