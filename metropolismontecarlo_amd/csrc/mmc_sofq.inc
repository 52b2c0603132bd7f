// mmc_sofq.inc -- host side of mmc_batch_structure_factor (include/mmc_hip.h, "Partial structure
// factors"; the kernels are in mmc_sofq.hpp).  Included by mmc_hip.hip after mmc_orient.inc; it shares
// the state checks of mmc_struct.inc and the device scratch of mmc_units.inc (obs_scratch).
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
    const size_t cnt_bytes = rep_bytes * (size_t)chunk, sum_bytes = sizeof(double) * n_ent;
    const size_t col_bytes = (sizeof(int32_t) * (size_t)n_cols + 15) & ~(size_t)15;
    char *d_buf = nullptr;
    MMC_TRY(obs_scratch(b, cnt_bytes + sum_bytes + col_bytes, &d_buf));
    std::vector<int64_t> h_sq(per_replica ? (size_t)R * n_ent : 0);
    std::vector<double> h_sum(per_replica ? 0 : n_ent);

    SofqArgs sa{};
    sa.box_r = s.pb.on ? s.pb.d_box : nullptr;
    sa.cnt = reinterpret_cast<unsigned long long *>(d_buf);
    double *d_sum = reinterpret_cast<double *>(d_buf + cnt_bytes);
    sa.cols = reinterpret_cast<const int32_t *>(d_buf + cnt_bytes + sum_bytes);
    sa.n_cols = n_cols;
    sa.S = S;

    const bool use_rec = struct_use_rec(b);
    const void *kern = use_rec ? reinterpret_cast<const void *>(k_sofq_wave<true>)
                               : reinterpret_cast<const void *>(k_sofq_wave<false>);
    hipStream_t st = s.stream;
    hipError_t e = hipSuccess;
    if (lds + 64 > 65536) // beyond what a workgroup may ask for without opting in: as k_recip_long_lds
        e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(s.lds_per_block - 64));
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_buf + cnt_bytes + sum_bytes, cols.data(), sizeof(int32_t) * (size_t)n_cols,
                           hipMemcpyHostToDevice, st);
    for (int64_t r0 = 0; r0 < R && e == hipSuccess; r0 += chunk) {
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
        e = hipMemsetAsync(d_buf, 0, rep_bytes * (size_t)n_rep, st);
        if (e != hipSuccess)
            break;
        if (use_rec)
            k_sofq_wave<true><<<(unsigned)wgs, SQ_WAVES * 64, lds, st>>>(s.bv, s.rec, sa);
        else
            k_sofq_wave<false><<<(unsigned)wgs, SQ_WAVES * 64, lds, st>>>(s.bv, nullptr, sa);
        e = hipGetLastError();
        if (e != hipSuccess)
            break;
        if (per_replica) {
            e = hipMemcpyAsync(h_sq.data() + (size_t)r0 * n_ent, d_buf, rep_bytes * (size_t)n_rep,
                               hipMemcpyDeviceToHost, st);
        } else {
            k_sofq_reduce<<<(unsigned)((n_ent + 255) / 256), 256, 0, st>>>(sa.cnt, d_sum, (int)n_rep, (int)n_ent,
                                                                          r0 == 0 ? 1 : 0);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess && !per_replica)
        e = hipMemcpyAsync(h_sum.data(), d_sum, sum_bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);
    else
        (void)hipStreamSynchronize(st); // (cols and the host arrays of copies already queued outlive them)
    MMC_REQUIRE(e == hipSuccess, MMC_ERR_HIP, "mmc_batch_structure_factor failed: %s", hipGetErrorString(e));
    // (the caller's arrays are written only on success)
    if (count)
        memcpy(count, h_count.data(), sizeof(int32_t) * (size_t)S);
    if (per_replica)
        memcpy(sq, h_sq.data(), sizeof(int64_t) * h_sq.size());
    else
        memcpy(sq_sum, h_sum.data(), sum_bytes);
    return MMC_OK;
}
