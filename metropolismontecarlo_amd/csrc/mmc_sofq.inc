// mmc_sofq.inc -- host side of mmc_batch_structure_factor (include/mmc_hip.h, "Partial structure
// factors"; the kernels are in mmc_sofq.hpp).  Included by mmc_hip.hip after mmc_units.inc (ObsCall).
#include "mmc_sofq.hpp"

#define SQ_CHUNK_BYTES ((size_t)256 << 20) // device scratch of the per-replica integers of one chunk

extern "C" int32_t mmc_batch_structure_factor(mmc_batch *b, int32_t n_max, int32_t per_replica, int32_t *count,
                                              int64_t *sq, double *sq_sum)
{
    // what can be refused without the batch comes first
    MMC_REQUIRE(n_max >= 1 && n_max <= MMC_SOFQ_MAX_N, MMC_ERR_ARG,
                "mmc_batch_structure_factor: n_max outside 1..%d", MMC_SOFQ_MAX_N);
    if (per_replica) {
        MMC_REQUIRE(sq, MMC_ERR_ARG, "mmc_batch_structure_factor: per_replica != 0 and sq is a NULL out pointer");
        MMC_REQUIRE(!sq_sum, MMC_ERR_ARG, "mmc_batch_structure_factor: per_replica != 0 takes no sq_sum");
    } else {
        MMC_REQUIRE(sq_sum, MMC_ERR_ARG, "mmc_batch_structure_factor: per_replica == 0 and sq_sum is a NULL out pointer");
        MMC_REQUIRE(!sq, MMC_ERR_ARG, "mmc_batch_structure_factor: per_replica == 0 takes no sq");
    }
    BATCH_CHECK(b);
    DeviceSystem &s = b->sys;
    const int64_t R = s.R;
    MMC_REQUIRE(per_replica || !s.pb.on, MMC_ERR_ARG,
                "mmc_batch_structure_factor: with per-replica boxes equal shells are different q: ask per replica");
    STRUCT_STATE(b);
    MMC_REQUIRE(s.n_mol >= 1 && s.n_mol <= MMC_SOFQ_MAX_MOL, MMC_ERR_UNSUPPORTED,
                "mmc_batch_structure_factor: 1 .. %d molecules (the phases of a replica stay in one workgroup's LDS)",
                MMC_SOFQ_MAX_MOL);
    const size_t lds = sizeof(double) * 18 * (size_t)s.n_mol;
    MMC_REQUIRE((int64_t)lds + 64 <= s.lds_per_block, MMC_ERR_UNSUPPORTED,
                "mmc_batch_structure_factor: the device grants %lld bytes of LDS per workgroup, %d molecules need %zu",
                (long long)s.lds_per_block, (int)s.n_mol, lds + 64);

    // shells, and the (nx, ny) columns of the half space with the largest |nz| of each, most work first
    const int n2 = n_max * n_max, S = n2 + 1;
    std::vector<int32_t> h_count((size_t)S, 0), cols;
    for (int kz = n_max; kz >= 0; kz--)
        for (int nx = 0; nx <= n_max; nx++)
            for (int ny = -n_max; ny <= n_max; ny++) {
                const int rem = n2 - nx * nx - ny * ny;
                if (rem < 0 || !(nx > 0 || ny >= 0))
                    continue;
                int m = 0;
                while ((m + 1) * (m + 1) <= rem)
                    m++;
                if (m != kz)
                    continue;
                cols.push_back(nx | (ny + 64) << 8 | m << 16);
                // the column's vectors and their mirror images
                for (int nz = -m; nz <= m; nz++)
                    if (nx > 0 || ny > 0 || nz > 0)
                        h_count[(size_t)(nx * nx + ny * ny + nz * nz)] += 2;
            }
    const int n_cols = (int)cols.size();

    const size_t n_ent = (size_t)6 * S, rep_bytes = sizeof(unsigned long long) * n_ent;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(R, (int64_t)(SQ_CHUNK_BYTES / rep_bytes)));
    const size_t sum_bytes = sizeof(double) * n_ent, col_bytes = sizeof(int32_t) * (size_t)n_cols;
    ObsCall oc(b);
    const size_t o_cnt = oc.take(rep_bytes * (size_t)chunk), o_sum = oc.take(sum_bytes), o_cols = oc.take(col_bytes);
    MMC_TRY(oc.alloc());

    SofqArgs sa{};
    sa.box_r = s.pb.on ? s.pb.d_box : nullptr;
    sa.cnt = oc.at<unsigned long long>(o_cnt);
    double *d_sum = oc.at<double>(o_sum);
    sa.cols = oc.at<int32_t>(o_cols);
    sa.n_cols = n_cols;
    sa.S = S;

    const bool use_rec = struct_use_rec(b);
    const void *kern = use_rec ? reinterpret_cast<const void *>(k_sofq_wave<true>)
                               : reinterpret_cast<const void *>(k_sofq_wave<false>);
    if (lds + 64 > 65536) // beyond what a workgroup may ask for without opting in: as k_recip_long_lds
        oc.e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(s.lds_per_block - 64));
    oc.to_device(oc.at<int32_t>(o_cols), cols.data(), col_bytes);
    for (int64_t r0 = 0; r0 < R && oc.e == hipSuccess; r0 += chunk) {
        const int64_t n_rep = std::min(chunk, R - r0);
        sa.r0 = (int32_t)r0;
        sa.n_rep = (int32_t)n_rep;
        // one workgroup per compute unit (its LDS, or its 256 registers per lane, leave room for no
        // second one).  Many replicas: persistent workgroups, a replica each at a time.  Fewer
        // replicas than compute units: `split` workgroups share a replica's columns.
        const int64_t cus = std::max(1, b->n_cus);
        sa.split = (int32_t)std::max<int64_t>(1, std::min<int64_t>(n_cols, cus / n_rep));
        const int64_t units = n_rep * sa.split;
        const int64_t wgs = std::max<int64_t>(1, std::min(b->wave_wgs > 0 ? (int64_t)b->wave_wgs : cus, units));
        oc.zero(rep_bytes * (size_t)n_rep);
        if (oc.e == hipSuccess) {
            if (use_rec)
                k_sofq_wave<true><<<(unsigned)wgs, SQ_WAVES * 64, lds, oc.st>>>(s.bv, s.rec, sa);
            else
                k_sofq_wave<false><<<(unsigned)wgs, SQ_WAVES * 64, lds, oc.st>>>(s.bv, nullptr, sa);
        }
        oc.launched();
        if (per_replica)
            oc.fetch(sq + (size_t)r0 * n_ent, sa.cnt, rep_bytes * (size_t)n_rep);
        else if (oc.e == hipSuccess)
            k_sofq_reduce<<<(unsigned)((n_ent + 255) / 256), 256, 0, oc.st>>>(sa.cnt, d_sum, (int)n_rep, (int)n_ent,
                                                                             r0 == 0 ? 1 : 0);
        oc.launched();
    }
    oc.fetch(sq_sum, d_sum, sum_bytes);
    MMC_TRY(oc.finish("mmc_batch_structure_factor"));
    if (count) // (as the other arrays of the caller: written only on success)
        memcpy(count, h_count.data(), sizeof(int32_t) * (size_t)S);
    return MMC_OK;
}
