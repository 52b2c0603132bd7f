// mmc_pair_energy.inc -- host side of mmc_batch_pair_energy (include/mmc_hip.h, "Pair-energy
// distributions"; the kernels are in mmc_pair_energy.hpp).  Included by mmc_hip.hip after
// mmc_orient.inc: it shares mmc_struct.inc's thresholds (rdf_thresholds) and state checks,
// mmc_units.inc's device scratch (obs_scratch) and mmc_deletion.inc's energy bins.
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
    double min_box = s.bv.box;
    if (s.pb.on) {
        MMC_REQUIRE(r_max > 0.0, MMC_ERR_ARG,
                    "mmc_batch_pair_energy: per-replica boxes have no common L/2: give r_max > 0");
        min_box = *std::min_element(s.pb.box.begin(), s.pb.box.end());
    }
    MMC_REQUIRE(!(r_max > 0.0) || r_max <= min_box / 2.0, MMC_ERR_ARG,
                "mmc_batch_pair_energy: r_max %g exceeds half of the smallest box %g", r_max, min_box);
    STRUCT_STATE(b);
    MMC_REQUIRE(s.uniform3, MMC_ERR_UNSUPPORTED, "mmc_batch_pair_energy: three-site molecules only");
    MMC_REQUIRE(s.n_mol >= 1 && s.n_mol <= (1 << 21), MMC_ERR_UNSUPPORTED,
                "mmc_batch_pair_energy: 1 .. 2^21 molecules (the tiles of a replica are counted in 32 bits)");

    // the bins of mmc_batch_rdf_sites: dr = side / 2 / numbins (gr.jl:5), else the caller's range
    const double dr = r_max > 0.0 ? r_max / numbins : (min_box / 2.0) / numbins;
    std::vector<double> thr;
    rdf_thresholds(dr, numbins, thr);

    // device scratch: the counter blocks of the kernel's LDS layout, the bond distribution, the
    // per-molecule counts (all zeroed), then the thresholds
    const size_t rs = (size_t)numbins + 2, e_slots = uhist ? (size_t)n_ebins + 2 : 0, ws = 3 * rs + e_slots + 1;
    const size_t n_or = per_replica ? (size_t)R : 1;
    const size_t out_bytes = 8 * n_or * ws, nhb_bytes = nhb ? 8 * n_or * MMC_PAIRE_NHB : 0;
    const size_t cnt_bytes = nhb ? (4 * (size_t)R * (size_t)s.n_mol + 7) / 8 * 8 : 0;
    // (thr carries the 18 LJ constants of the record instantiation behind the thresholds)
    double h_lj[18] = { 0.0 };
    const size_t zero_bytes = out_bytes + nhb_bytes + cnt_bytes, thr_bytes = sizeof(double) * (thr.size() + 18);
    char *d_buf = nullptr;
    MMC_TRY(obs_scratch(b, zero_bytes + thr_bytes, &d_buf));
    std::vector<unsigned long long> h_out((out_bytes + nhb_bytes) / 8);

    PairEArgs pa{};
    pa.out = reinterpret_cast<unsigned long long *>(d_buf);
    unsigned long long *d_nhb = reinterpret_cast<unsigned long long *>(d_buf + out_bytes);
    pa.cnt = nhb ? reinterpret_cast<int32_t *>(d_buf + out_bytes + nhb_bytes) : nullptr;
    pa.thr = reinterpret_cast<const double *>(d_buf + zero_bytes);
    pa.lj = pa.thr + thr.size();
    pa.box_r = s.pb.on ? s.pb.d_box : nullptr;
    pa.numbins = numbins;
    pa.per_replica = per_replica ? 1 : 0;
    pa.e_slots = (int32_t)e_slots;
    pa.wstride = (int32_t)ws;
    pa.inv_dr = (float)(1.0 / dr);
    const int64_t K = (s.n_mol + 63) / 64;
    pa.n_blocks = (int32_t)K;
    pa.tiles_per_rep = (int32_t)(K * (K + 1) / 2);
    pa.n_tiles = R * pa.tiles_per_rep;
    pa.u_lo = uhist ? u_lo : 0.0;
    pa.u_hi = uhist ? u_hi : 1.0;
    pa.scale = uhist ? (double)n_ebins / (u_hi - u_lo) : 0.0;
    pa.u_hb = nhb ? u_hb : 0.0;
    pa.factor = s.bv.factor;
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

    // waves per workgroup: as many of PE_WAVES as have room for their counters beside the thresholds
    int nw = PE_WAVES;
    while (nw > 1 && 8 * rs + PE_LJ_BYTES + (size_t)nw * 8 * ws > PE_LDS_BYTES)
        nw >>= 1;
    const size_t lds = 8 * rs + PE_LJ_BYTES + (size_t)nw * 8 * ws;
    // persistent workgroups: four waves per SIMD of every compute unit, or option "wave_wgs"; no more
    // than there are tiles
    int64_t wgs = b->wave_wgs > 0 ? b->wave_wgs : (int64_t)(16 / nw) * b->n_cus;
    wgs = std::max<int64_t>(1, std::min(wgs, (pa.n_tiles + nw - 1) / nw));

    hipStream_t st = s.stream;
    thr.insert(thr.end(), h_lj, h_lj + 18);
    hipError_t e = hipMemsetAsync(d_buf, 0, zero_bytes, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_buf + zero_bytes, thr.data(), thr_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        if (use_rec)
            k_pair_energy_wave<true><<<(unsigned)wgs, nw * 64, lds, st>>>(s.bv, s.rec, pa);
        else
            k_pair_energy_wave<false><<<(unsigned)wgs, nw * 64, lds, st>>>(s.bv, nullptr, pa);
        e = hipGetLastError();
    }
    if (e == hipSuccess && nhb) {
        const unsigned g = (unsigned)std::min<int64_t>(R, (int64_t)4 * std::max(1, b->n_cus));
        k_pair_energy_nhb<<<g, 256, 0, st>>>(pa.cnt, (int)s.n_mol, (int)R, pa.per_replica, d_nhb);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(h_out.data(), d_buf, out_bytes + nhb_bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);
    else
        (void)hipStreamSynchronize(st); // (thr and h_out of copies already queued outlive them)
    MMC_REQUIRE(e == hipSuccess, MMC_ERR_HIP, "mmc_batch_pair_energy failed: %s", hipGetErrorString(e));
    // (the caller's arrays are written only on success)
    for (size_t r = 0; r < n_or; r++) {
        const unsigned long long *blk = h_out.data() + r * ws;
        memcpy(rows + r * 3 * rs, blk, 8 * 3 * rs);
        if (uhist)
            memcpy(uhist + r * e_slots, blk + 3 * rs, 8 * e_slots);
        flagged[r] = blk[3 * rs + e_slots];
    }
    if (nhb)
        memcpy(nhb, h_out.data() + n_or * ws, nhb_bytes);
    return MMC_OK;
}
