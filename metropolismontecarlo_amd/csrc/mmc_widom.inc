// mmc_widom.inc -- host side of Widom test-particle insertion (include/mmc_hip.h, "Widom
// test-particle insertion"; the kernels are in mmc_widom.hpp).  Included by mmc_hip.hip after
// mmc_units.inc, which holds what the call shares with mmc_deletion.inc and mmc_forces.inc: the state
// checks, the device scratch and pinned staging, the launch and the drain of the stream.  InsertionCall,
// here, is what the call shares with mmc_solute.inc from the staging of the sums to the caller's arrays.
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

// An insertion call (mmc_batch_widom / _widom_at here, mmc_batch_widom_solute / _solute_at in
// mmc_solute.inc): a unit call with terms [R M][4], flags [R M], one sum and one count per replica,
// then the inserted species' parameters and, where the caller gives or wants them, the placements
// [R M][words].  begin(), the caller's launch() of its unit kernel, finish().
struct InsertionCall : UnitsCall {
    size_t par_bytes, mol_bytes, o_par, o_mol;

    InsertionCall(mmc_batch *b_, size_t n_units, size_t par_bytes_, size_t mol_bytes_)
        : UnitsCall(b_, n_units, 4, 1), par_bytes(par_bytes_), mol_bytes(mol_bytes_)
    {
        o_par = take(par_bytes);
        o_mol = take(mol_bytes);
    }
    double *d_par() const { return at<double>(o_par); }
    double *d_mol() const { return mol_bytes ? at<double>(o_mol) : nullptr; }

    // after alloc(): the caller's sums into the staged block, and what the unit kernel reads to the
    // device (h_par, mol_in: NULL = the kernel does not read them).  From here to finish() nothing returns.
    void begin(const double *boltz_sum, const int64_t *n_overlap, const double *h_par, const double *mol_in)
    {
        memcpy(h_sums(), boltz_sum, sizeof(double) * R);
        memcpy(h_counts(), n_overlap, sizeof(long long) * R);
        upload_block();
        if (h_par)
            to_device(d_par(), h_par, par_bytes);
        if (mol_in)
            to_device(d_mol(), mol_in, mol_bytes);
    }
    // after launch(): k_widom_reduce adds every replica's M terms to its sums, the stream is drained,
    // and the caller's arrays are written only once the whole call has succeeded
    int32_t finish(int64_t M, double temperature, double *boltz_sum, int64_t *n_overlap, double *mol_out, double *du_out,
                   uint8_t *ovl_out, const char *what)
    {
        if (e == hipSuccess)
            k_widom_reduce<<<(unsigned)R, 64, 0, st>>>(d_rows(), d_flags(), (int)M, 1.0 / temperature, d_sums(), d_counts());
        launched();
        std::vector<double> h_terms, h_mol(mol_out ? mol_bytes / sizeof(double) : 0);
        std::vector<uint8_t> h_flags;
        if (mol_out)
            to_host(h_mol.data(), d_mol(), mol_bytes);
        MMC_TRY(UnitsCall::finish(du_out ? &h_terms : nullptr, ovl_out ? &h_flags : nullptr, what));
        memcpy(boltz_sum, h_sums(), sizeof(double) * R);
        memcpy(n_overlap, h_counts(), sizeof(long long) * R);
        if (du_out)
            for (size_t i = 0; i < nu; i++)
                for (int c = 0; c < 3; c++)
                    du_out[3 * i + c] = h_terms[4 * i + c];
        if (ovl_out)
            memcpy(ovl_out, h_flags.data(), nu);
        if (mol_out)
            memcpy(mol_out, h_mol.data(), mol_bytes);
        return MMC_OK;
    }
};

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
    MMC_TRY(temperature_arg(temperature, what));
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

    // ---- device scratch: the parameters are the offsets [9], a placement the molecule [12] ----
    const size_t n = (size_t)(R * M);
    InsertionCall uc(b, n, sizeof(double) * 9, (mol_in || mol_out) ? sizeof(double) * 12 * n : 0);
    MMC_TRY(uc.alloc());

    WidomArgs wa{};
    wa.seed = seed;
    wa.draw0 = draw0;
    wa.off = uc.d_par();
    wa.mol_in = mol_in ? uc.d_mol() : nullptr;
    wa.mol_out = (!mol_in && mol_out) ? uc.d_mol() : nullptr;
    wa.terms = uc.d_rows();
    wa.flags = uc.d_flags();
    wa.scur = uc.d_scur();
    wa.n_insert = (int32_t)M;
    wa.self_d = ewald_self_term(s.fc.q, 3, s.bv.kappa, s.bv.factor); // EwaldSelf(N+1) - EwaldSelf(N)

    const PairParams pp = mmc_pair_params(b->lj_rcut, b->qq_rcut, 0.0, 0.5, s.bv.kappa, false);
    // the minimum image of an atom pair from its molecules' (WV_IMG): k_move_eval_wave's condition with
    // the test molecule's extent in place of one r_mol_max, gate + r_mol + r_test < box / 2 and inside
    // the slack of the pair tests, where the chains' molecules are known to be rigid.  (Not
    // units_image_by_molecule: a different expression in fp64, and r_test is this call's own.)
    const double far = std::sqrt(std::max(pp.lj_gate_sq, pp.qq_gate_sq)) + s.r_mol_max + r_test + 1e-6;
    const bool img = b->rigid_only && b->image_by_molecule != 0 && std::isfinite(far) && far < 0.5 * s.box &&
                     far * far < pp.qq_slack_sq && far * far < pp.lj_slack_sq;

    uc.begin(boltz_sum, n_overlap, offsets, mol_in);
    uc.launch(img, k_widom_wave<true>, k_widom_wave<false>, WIDOM_OCC, pp, wa);
    return uc.finish(M, temperature, boltz_sum, n_overlap, mol_out, du_out, ovl_out, what);
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
