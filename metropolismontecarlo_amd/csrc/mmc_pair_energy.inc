// mmc_pair_energy.inc -- host side of mmc_batch_pair_energy (include/mmc_hip.h, "Pair-energy
// distributions"; the kernels are in mmc_pair_energy.hpp).  Included by mmc_hip.hip after
// mmc_units.inc (ObsCall, tile_plan: the bins are mmc_batch_rdf_sites') and mmc_deletion.inc, whose
// energy bins it shares.
#include "mmc_pair_energy.hpp"

static_assert(MMC_PAIRE_MAX_EBINS == MMC_DELETION_MAX_BINS, "the energy bins are mmc_batch_deletion's");

extern "C" int32_t mmc_batch_pair_energy(mmc_batch *b, int32_t numbins, double r_max, int32_t n_ebins, double u_lo,
                                         double u_hi, double u_hb, int32_t per_replica, int64_t *rows,
                                         uint64_t *uhist, uint64_t *nhb, uint64_t *flagged)
{
    // what can be refused without the batch comes first
    MMC_REQUIRE(rows, MMC_ERR_ARG, "mmc_batch_pair_energy: NULL rows pointer");
    MMC_REQUIRE(flagged, MMC_ERR_ARG, "mmc_batch_pair_energy: NULL flagged pointer");
    MMC_REQUIRE(numbins >= 1 && numbins <= MMC_PAIRE_MAX_BINS, MMC_ERR_ARG,
                "mmc_batch_pair_energy: numbins outside 1..%d", MMC_PAIRE_MAX_BINS);
    MMC_REQUIRE(std::isfinite(r_max), MMC_ERR_ARG, "mmc_batch_pair_energy: r_max is not finite");
    if (uhist) {
        MMC_REQUIRE(n_ebins >= 1 && n_ebins <= MMC_PAIRE_MAX_EBINS, MMC_ERR_ARG,
                    "mmc_batch_pair_energy: n_ebins outside 1..%d", MMC_PAIRE_MAX_EBINS);
        MMC_REQUIRE(std::isfinite(u_lo) && std::isfinite(u_hi) && u_lo < u_hi, MMC_ERR_ARG,
                    "mmc_batch_pair_energy: uhist wants finite u_lo < u_hi");
    }
    MMC_REQUIRE(!nhb || std::isfinite(u_hb), MMC_ERR_ARG, "mmc_batch_pair_energy: u_hb is not finite");
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    const int64_t R = s.R;
    PairEArgs pa{};
    std::vector<double> thr;
    MMC_TRY(tile_plan(b, numbins, r_max, "mmc_batch_pair_energy", &pa.ta, &thr));
    MMC_REQUIRE(s.uniform3, MMC_ERR_UNSUPPORTED, "mmc_batch_pair_energy: three-site molecules only");
    BATCH_NO_SOLUTE(b, "mmc_batch_pair_energy");
    pa.ta.per_replica = per_replica ? 1 : 0;

    const size_t rs = (size_t)numbins + 2, e_slots = uhist ? (size_t)n_ebins + 2 : 0, ws = 3 * rs + e_slots + 1;
    pa.e_slots = (int32_t)e_slots;
    pa.wstride = (int32_t)ws;
    pa.u_lo = uhist ? u_lo : 0.0;
    pa.u_hi = uhist ? u_hi : 1.0;
    pa.scale = uhist ? (double)n_ebins / (u_hi - u_lo) : 0.0;
    pa.u_hb = nhb ? u_hb : 0.0;
    pa.factor = s.bv.factor;
    // (thr carries the 18 LJ constants of the record instantiation behind the thresholds)
    double h_lj[18] = { 0.0 };
    const bool use_rec = struct_use_rec(b);
    if (use_rec) { // every molecule is a copy of the first: its nine atom pairs are launch constants
        for (int ab = 0; ab < 9; ab++) {
            h_lj[2 * ab] = 4.0 * s.fc.eps9[ab];
            h_lj[2 * ab + 1] = s.fc.sig9[ab] * s.fc.sig9[ab];
        }
        for (int a = 0; a < 3; a++)
            pa.q3[a] = s.fc.q[a];
        pa.lj_mask = s.fc.lj_mask;
    }
    thr.insert(thr.end(), h_lj, h_lj + 18);

    // waves per workgroup: the thresholds and the LJ constants, and a block of counters a wave
    const int nw = tile_waves(8 * rs + PE_LJ_BYTES, 8 * ws);
    const size_t lds = 8 * rs + PE_LJ_BYTES + (size_t)nw * 8 * ws;
    const unsigned wgs = obs_grid(b, nw, pa.ta.n_tiles);

    // device scratch: the counter blocks of the kernel's LDS layout, the bond distribution, the
    // per-molecule counts (all zeroed), then the thresholds
    ObsCall oc(b);
    const size_t n_or = per_replica ? (size_t)R : 1;
    const size_t out_bytes = 8 * n_or * ws, nhb_bytes = nhb ? 8 * n_or * MMC_PAIRE_NHB : 0;
    const size_t o_out = oc.take(out_bytes), o_nhb = oc.take(nhb_bytes),
                 o_cnt = oc.take(nhb ? 4 * (size_t)R * (size_t)s.n_mol : 0), o_thr = oc.take(sizeof(double) * thr.size());
    MMC_TRY(oc.alloc());
    pa.out = oc.at<unsigned long long>(o_out);
    unsigned long long *d_nhb = oc.at<unsigned long long>(o_nhb);
    pa.cnt = nhb ? oc.at<int32_t>(o_cnt) : nullptr;
    pa.ta.thr = oc.at<double>(o_thr);
    pa.lj = pa.ta.thr + (thr.size() - 18);

    oc.zero(o_thr);
    oc.to_device(oc.at<double>(o_thr), thr.data(), sizeof(double) * thr.size());
    if (oc.e == hipSuccess) {
        if (use_rec)
            k_pair_energy_wave<true><<<wgs, nw * 64, lds, oc.st>>>(s.bv, s.rec, pa);
        else
            k_pair_energy_wave<false><<<wgs, nw * 64, lds, oc.st>>>(s.bv, nullptr, pa);
    }
    oc.launched();
    if (oc.e == hipSuccess && nhb) {
        const unsigned g = (unsigned)std::min<int64_t>(R, (int64_t)4 * std::max(1, b->n_cus));
        k_pair_energy_nhb<<<g, 256, 0, oc.st>>>(pa.cnt, (int)s.n_mol, (int)R, pa.ta.per_replica, d_nhb);
    }
    oc.launched();
    const unsigned long long *h_out = reinterpret_cast<const unsigned long long *>(oc.stage(pa.out, out_bytes));
    oc.fetch(nhb, d_nhb, nhb_bytes);
    MMC_TRY(oc.finish("mmc_batch_pair_energy"));
    // (the caller's arrays are written only on success)
    for (size_t r = 0; r < n_or; r++) {
        const unsigned long long *blk = h_out + r * ws;
        memcpy(rows + r * 3 * rs, blk, 8 * 3 * rs);
        if (uhist)
            memcpy(uhist + r * e_slots, blk + 3 * rs, 8 * e_slots);
        flagged[r] = blk[3 * rs + e_slots];
    }
    return MMC_OK;
}
