// mmc_solute.inc -- host side of Widom insertion of foreign rigid solutes (include/mmc_hip.h,
// "Foreign solutes"; the kernel is in mmc_solute.hpp, the reduce kernel is mmc_widom.hpp's).
// Included by mmc_hip.hip after mmc_widom.inc, whose InsertionCall is the call from the staging of the
// sums to the caller's arrays; the solute's record, refusals and parameter rows, the state checks, the
// scratch, the launch and the drain of the stream are mmc_units.inc's.
#include "mmc_solute.hpp"

static int32_t solute_run(mmc_batch *b, const SoluteIn &sol, int64_t M, uint64_t seed, int64_t draw0, const double *mol_in,
                          bool at, double temperature, double *boltz_sum, int64_t *n_overlap, double *mol_out,
                          double *du_out, uint8_t *ovl_out, const char *what)
{
    // ---- arguments (MMC_ERR_ARG): first what needs no batch, so that it is refused without a device;
    // then state (MMC_ERR_STATE), then scope (MMC_ERR_UNSUPPORTED); nothing is written before every
    // check has passed ----
    const int32_t S = sol.S;
    MMC_REQUIRE(S >= 1 && S <= SOL_MAX_SITES, MMC_ERR_ARG, "%s: n_sites must be 1..%d", what, SOL_MAX_SITES);
    MMC_TRY(solute_null_args(sol, what));
    if (at)
        MMC_REQUIRE(mol_in, MMC_ERR_ARG, "%s: NULL mol_in", what);
    else
        MMC_REQUIRE(sol.offsets, MMC_ERR_ARG, "%s: NULL offsets", what);
    MMC_REQUIRE(boltz_sum && n_overlap, MMC_ERR_ARG, "%s: boltz_sum and n_overlap are required", what);
    MMC_REQUIRE(M >= 1, MMC_ERR_ARG, "%s: n_insert must be >= 1", what);
    MMC_TRY(temperature_arg(temperature, what));
    bool charged = false;
    double q2;
    MMC_TRY(solute_value_args(sol, what, &charged, &q2));
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    const int64_t R = s.R, nw = 3 * (int64_t)S + 3;
    MMC_REQUIRE(R * M <= (int64_t)INT32_MAX, MMC_ERR_ARG, "%s: replicas x n_insert exceeds 2^31 - 1", what);
    if (at)
        for (int64_t k = 0; k < R * M * nw; k++)
            MMC_REQUIRE(std::isfinite(mol_in[k]), MMC_ERR_ARG, "%s: non-finite mol_in", what);
    MMC_TRY(units_state_scope(b, what));

    // ---- device scratch: the parameters are the solute [S][SOL_PAR], a placement its sites and
    // reference point [S + 1][3] ----
    const size_t n = (size_t)(R * M);
    InsertionCall uc(b, n, sizeof(double) * SOL_PAR * S, (at || mol_out) ? sizeof(double) * nw * n : 0);
    MMC_TRY(uc.alloc());
    std::vector<double> h_par((size_t)SOL_PAR * S, 0.0);
    solute_pack(h_par.data(), sol, sol.offsets);

    SoluteArgs sa{};
    sa.seed = seed;
    sa.draw0 = draw0;
    sa.par = uc.d_par();
    sa.mol_in = at ? uc.d_mol() : nullptr;
    sa.mol_out = (!at && mol_out) ? uc.d_mol() : nullptr;
    sa.terms = uc.d_rows();
    sa.flags = uc.d_flags();
    sa.scur = uc.d_scur();
    sa.n_insert = (int32_t)M;
    sa.n_sites = S;
    sa.self_d = ewald_self_term(sol.charge, S, s.bv.kappa, s.bv.factor); // EwaldSelf(N+1) - EwaldSelf(N)
    const PairParams pp = mmc_pair_params(b->lj_rcut, b->qq_rcut, 0.0, 0.5, s.bv.kappa, false);
    // the instantiation: no reciprocal part for an uncharged solute, else the smallest phase tables
    const units_kernel_t<SoluteArgs> kern = !charged ? k_solute_wave<0> : S <= 4 ? k_solute_wave<4> : k_solute_wave<16>;
    const int occ = !charged ? SOL_OCC(0) : S <= 4 ? SOL_OCC(4) : SOL_OCC(16);

    uc.begin(boltz_sum, n_overlap, h_par.data(), at ? mol_in : nullptr);
    uc.launch(false, kern, kern, occ, pp, sa);
    return uc.finish(M, temperature, boltz_sum, n_overlap, mol_out, du_out, ovl_out, what);
}

extern "C" int32_t mmc_batch_widom_solute(mmc_batch *b, int32_t n_sites, const double *offsets, const double *charge,
                                          const double *eps, const double *sig, int64_t n_insert, uint64_t seed,
                                          int64_t draw0, double temperature, double *boltz_sum, int64_t *n_overlap,
                                          double *mol_out, double *du_out, uint8_t *ovl_out)
{
    return solute_run(b, SoluteIn{ n_sites, offsets, charge, eps, sig, "" }, n_insert, seed, draw0, nullptr, false,
                      temperature, boltz_sum, n_overlap, mol_out, du_out, ovl_out, "mmc_batch_widom_solute");
}

extern "C" int32_t mmc_batch_widom_solute_at(mmc_batch *b, int32_t n_sites, const double *charge, const double *eps,
                                             const double *sig, int64_t n_insert, const double *mol_in,
                                             double temperature, double *boltz_sum, int64_t *n_overlap,
                                             double *du_out, uint8_t *ovl_out)
{
    return solute_run(b, SoluteIn{ n_sites, nullptr, charge, eps, sig, "" }, n_insert, 0, 0, mol_in, true, temperature,
                      boltz_sum, n_overlap, nullptr, du_out, ovl_out, "mmc_batch_widom_solute_at");
}
