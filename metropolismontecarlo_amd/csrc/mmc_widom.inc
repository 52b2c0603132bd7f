// mmc_widom.inc -- host side of Widom test-particle insertion (include/mmc_hip.h, "Widom
// test-particle insertion"; the kernels are in mmc_widom.hpp).  Included by mmc_hip.hip after
// mmc_units.inc, which holds what the call shares with mmc_deletion.inc and mmc_forces.inc: the state
// checks, the device scratch and pinned staging, the launch and the drain of the stream.
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
    MMC_TRY(units_state_scope(b, what));

    // ---- device scratch: terms [R M][4], flags [R M], the per-replica block (sums [R], counts [R]),
    // offsets [9], molecules [R M][12] ----
    const size_t n = (size_t)(R * M);
    const bool need_mol = mol_in || mol_out;
    UnitsCall uc(b, n, 4, 1);
    const size_t o_off = uc.take(sizeof(double) * 9), o_mol = uc.take(need_mol ? sizeof(double) * 12 * n : 0);
    MMC_TRY(uc.alloc());
    double *d_off = uc.at<double>(o_off), *d_mol = need_mol ? uc.at<double>(o_mol) : nullptr;
    memcpy(uc.h_sums(), boltz_sum, sizeof(double) * R);
    memcpy(uc.h_counts(), n_overlap, sizeof(long long) * R);

    WidomArgs wa{};
    wa.seed = seed;
    wa.draw0 = draw0;
    wa.off = d_off;
    wa.mol_in = mol_in ? d_mol : nullptr;
    wa.mol_out = (!mol_in && mol_out) ? d_mol : nullptr;
    wa.terms = uc.d_rows();
    wa.flags = uc.d_flags();
    wa.scur = uc.d_scur();
    wa.n_insert = (int32_t)M;
    {   // EwaldSelf(N+1) - EwaldSelf(N) in orc_ewald_self's arithmetic (ewalds.jl:829-833)
        double q2 = 0.0;
        for (int a = 0; a < 3; a++)
            q2 += s.fc.q[a] * s.fc.q[a];
        wa.self_d = -s.bv.kappa * q2 / std::sqrt(M_PI) * s.bv.factor;
    }

    const PairParams pp = mmc_pair_params(b->lj_rcut, b->qq_rcut, 0.0, 0.5, s.bv.kappa, false);
    // the minimum image of an atom pair from its molecules' (WV_IMG): k_move_eval_wave's condition with
    // the test molecule's extent in place of one r_mol_max, gate + r_mol + r_test < box / 2 and inside
    // the slack of the pair tests, where the chains' molecules are known to be rigid.  (Not
    // units_image_by_molecule: a different expression in fp64, and r_test is this call's own.)
    const double far = std::sqrt(std::max(pp.lj_gate_sq, pp.qq_gate_sq)) + s.r_mol_max + r_test + 1e-6;
    const bool img = b->rigid_only && b->image_by_molecule != 0 && std::isfinite(far) && far < 0.5 * s.box &&
                     far * far < pp.qq_slack_sq && far * far < pp.lj_slack_sq;

    // ---- from here to finish() nothing returns ----
    uc.upload_block();
    if (offsets)
        uc.to_device(d_off, offsets, sizeof(double) * 9);
    if (mol_in)
        uc.to_device(d_mol, mol_in, sizeof(double) * 12 * n);
    uc.launch(img, k_widom_wave<true>, k_widom_wave<false>, WIDOM_OCC, pp, wa);
    if (uc.e == hipSuccess)
        k_widom_reduce<<<(unsigned)R, 64, 0, uc.st>>>(uc.d_rows(), uc.d_flags(), (int)M, 1.0 / temperature, uc.d_sums(),
                                                     uc.d_counts());
    uc.launched();
    std::vector<double> h_terms, h_mol(mol_out ? 12 * n : 0);
    std::vector<uint8_t> h_flags;
    if (mol_out)
        uc.to_host(h_mol.data(), d_mol, sizeof(double) * 12 * n);
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
