// mmc_struct.inc -- host side of the structure observables (include/mmc_hip.h, "Structure
// observables"; the kernels are in mmc_struct.hpp).  Included by mmc_hip.hip after mmc_units.inc,
// whose device scratch (obs_scratch) both calls use.
#include "mmc_struct.hpp"

// gr.jl:87 on r^2, in the arithmetic of k_rdf: the bin of a squared distance
static inline double rdf_bin_of(double r2, double dr)
{
    return std::ceil(std::sqrt(r2) / dr);
}

// thr[k], k = 0 .. numbins: the largest double r^2 >= 0 with rdf_bin_of(r^2) <= k (the bin is
// monotone in r^2: sqrt, the division by dr > 0 and ceil are), found by bisection over the bit
// patterns of the non-negative doubles; thr[numbins + 1] = +inf.
static void rdf_thresholds(double dr, int numbins, std::vector<double> &thr)
{
    auto bits = [](double x) { uint64_t u; memcpy(&u, &x, 8); return u; };
    auto dbl = [](uint64_t u) { double x; memcpy(&x, &u, 8); return x; };
    thr.assign((size_t)numbins + 2, INFINITY);
    for (int k = 0; k <= numbins; k++) {
        const double e = dr * (k + 1);
        uint64_t lo = 0, hi = bits(e * e * 1.01); // bin(0) = 0 <= k; bin(hi) >= k + 2
        if (!(rdf_bin_of(dbl(hi), dr) > k)) {     // (dr so large that the bound overflowed: nothing is beyond)
            thr[k] = INFINITY;
            continue;
        }
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (rdf_bin_of(dbl(mid), dr) <= k)
                lo = mid;
            else
                hi = mid;
        }
        thr[k] = dbl(lo);
    }
}

// preconditions of both calls (those of mmc_batch_potential_ewald)
#define STRUCT_STATE(b)                                                                          \
    MMC_REQUIRE(!(b)->has_prev, MMC_ERR_STATE, "proposals outstanding: call mmc_batch_settle first"); \
    BATCH_NO_VOLUME_TRIAL(b)

// the 128-byte records where the batch keeps them in step with the coordinates (as the totals do)
static inline bool struct_use_rec(const mmc_batch *b)
{
    return b->sys.rec && b->sys.homogeneous && (b->sys.pb.on || b->fast_ok);
}

extern "C" int32_t mmc_batch_rdf_sites(mmc_batch *b, int32_t numbins, double r_max, int32_t per_replica,
                                       uint64_t *hist)
{
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    const int64_t R = s.R;
    MMC_REQUIRE(hist, MMC_ERR_ARG, "mmc_batch_rdf_sites: NULL out pointer");
    MMC_REQUIRE(numbins >= 1 && numbins <= MMC_RDF_SITES_MAX_BINS, MMC_ERR_ARG,
                "mmc_batch_rdf_sites: numbins outside 1..%d", MMC_RDF_SITES_MAX_BINS);
    MMC_REQUIRE(std::isfinite(r_max), MMC_ERR_ARG, "mmc_batch_rdf_sites: r_max is not finite");
    double min_box = s.bv.box;
    if (s.pb.on) {
        MMC_REQUIRE(r_max > 0.0, MMC_ERR_ARG,
                    "mmc_batch_rdf_sites: per-replica boxes have no common L/2: give r_max > 0");
        min_box = *std::min_element(s.pb.box.begin(), s.pb.box.end());
    }
    MMC_REQUIRE(!(r_max > 0.0) || r_max <= min_box / 2.0, MMC_ERR_ARG,
                "mmc_batch_rdf_sites: r_max %g exceeds half of the smallest box %g", r_max, min_box);
    STRUCT_STATE(b);
    MMC_REQUIRE(s.n_mol >= 1 && s.n_mol <= (1 << 21), MMC_ERR_UNSUPPORTED,
                "mmc_batch_rdf_sites: 1 .. 2^21 molecules (the tiles of a replica are counted in 32 bits)");
    // (a batch holds three-atom molecules only, mmc_batch_create: slots 0..2 exist in every molecule)

    // gr.jl:5: dr = side / 2 / numbins; else the caller's range
    const double dr = r_max > 0.0 ? r_max / numbins : (min_box / 2.0) / numbins;
    std::vector<double> thr;
    rdf_thresholds(dr, numbins, thr);

    const size_t n_out = (size_t)(per_replica ? R : 1) * 6 * (size_t)(numbins + 1);
    const size_t hist_bytes = sizeof(unsigned long long) * n_out, thr_bytes = sizeof(double) * thr.size();
    char *d_buf = nullptr;
    MMC_TRY(obs_scratch(b, hist_bytes + thr_bytes, &d_buf));
    std::vector<uint64_t> h_out(n_out);

    RdfSitesArgs sa{};
    sa.thr = reinterpret_cast<const double *>(d_buf + hist_bytes);
    sa.box_r = s.pb.on ? s.pb.d_box : nullptr;
    sa.hist = reinterpret_cast<unsigned long long *>(d_buf);
    sa.numbins = numbins;
    sa.per_replica = per_replica ? 1 : 0;
    sa.inv_dr = (float)(1.0 / dr);
    const int64_t K = (s.n_mol + 63) / 64;
    sa.n_blocks = (int32_t)K;
    sa.tiles_per_rep = (int32_t)(K * (K + 1) / 2);
    sa.n_tiles = R * sa.tiles_per_rep;

    // waves per workgroup: as many of ST_WAVES as have room for their histograms beside the thresholds
    const size_t rs = (size_t)numbins + 2;
    int nw = ST_WAVES;
    while (nw > 1 && 8 * rs + (size_t)nw * 24 * rs > ST_LDS_BYTES)
        nw >>= 1;
    const size_t lds = 8 * rs + (size_t)nw * 24 * rs;
    // persistent workgroups: four waves per SIMD of every compute unit (the pass is bound by vector
    // issue), or option "wave_wgs"; no more than there are tiles
    int64_t wgs = b->wave_wgs > 0 ? b->wave_wgs : (int64_t)(16 / nw) * b->n_cus;
    wgs = std::max<int64_t>(1, std::min(wgs, (sa.n_tiles + nw - 1) / nw));

    hipStream_t st = s.stream;
    hipError_t e = hipMemsetAsync(d_buf, 0, hist_bytes, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_buf + hist_bytes, thr.data(), thr_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        if (struct_use_rec(b))
            k_rdf_sites_wave<true><<<(unsigned)wgs, nw * 64, lds, st>>>(s.bv, s.rec, sa);
        else
            k_rdf_sites_wave<false><<<(unsigned)wgs, nw * 64, lds, st>>>(s.bv, nullptr, sa);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(h_out.data(), d_buf, hist_bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);
    MMC_REQUIRE(e == hipSuccess, MMC_ERR_HIP, "mmc_batch_rdf_sites failed: %s", hipGetErrorString(e));
    memcpy(hist, h_out.data(), hist_bytes); // (the caller's array is written only on success)
    return MMC_OK;
}

extern "C" int32_t mmc_batch_dipoles(mmc_batch *b, double *dip)
{
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    const int64_t R = s.R;
    MMC_REQUIRE(dip, MMC_ERR_ARG, "mmc_batch_dipoles: NULL out pointer");
    STRUCT_STATE(b);
    const size_t bytes = sizeof(double) * 3 * (size_t)R;
    char *d_buf = nullptr;
    MMC_TRY(obs_scratch(b, bytes, &d_buf));
    double *d_dip = reinterpret_cast<double *>(d_buf);
    std::vector<double> h_out(3 * (size_t)R);
    hipStream_t st = s.stream;
    const unsigned wgs = (unsigned)((R + ST_WAVES - 1) / ST_WAVES);
    const double *box_r = s.pb.on ? s.pb.d_box : nullptr;
    if (struct_use_rec(b))
        k_dipoles<true><<<wgs, ST_WAVES * 64, 0, st>>>(s.bv, s.rec, box_r, d_dip, (int)R);
    else
        k_dipoles<false><<<wgs, ST_WAVES * 64, 0, st>>>(s.bv, nullptr, box_r, d_dip, (int)R);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipMemcpyAsync(h_out.data(), d_dip, bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);
    MMC_REQUIRE(e == hipSuccess, MMC_ERR_HIP, "mmc_batch_dipoles failed: %s", hipGetErrorString(e));
    memcpy(dip, h_out.data(), bytes);
    return MMC_OK;
}
