// mmc_system.inc -- DeviceSystem: device-resident replica state, uploads, Ewald tables, totals.
// Included by mmc_hip.hip (single translation unit).

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>

static thread_local char g_err[512] = "";

void mmc_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char *mmc_last_error(void) { return g_err; }
extern "C" const char *mmc_version(void) { return "mmc-hip 0.1 (gfx950)"; }

extern "C" int32_t mmc_device_count(int32_t *count)
{
    MMC_REQUIRE(count, MMC_ERR_ARG, "count is NULL");
    int n = 0;
    MMC_HIP(hipGetDeviceCount(&n));
    *count = n;
    return MMC_OK;
}

// PrepareEwaldVariables (ewalds.jl:45-103) on the device: one wave walks the (nk+1)(2nk+1)^2
// candidates in the reference's nesting order (kx outer, kz inner) and compacts the survivors of
// `0 < k^2 < k_sq_max` with ballot + prefix, so kxyz/cfac come out in the reference's order.
// k_sq_max == 27 (asserted by the caller) bounds |k| <= 5, so a fixed 6 x 11 x 11 walk is complete.
//
// half != 0 (a batch: its structure factors are always the library's own sums over coordinates,
// never arrays a caller hands in): the list WITHOUT the later member of each conjugate pair of the
// kx = 0 plane.  The reference keeps both (0, ky, kz) and (0, -ky, -kz) -- it halves only kx > 0
// (ewalds.jl:81-83) -- and S of the second is the conjugate of S of the first bit for bit (negative
// table indices ARE conjugates, ewalds.jl:575-585; products and sums of conjugates are conjugates in
// IEEE arithmetic; tests/test_oracle.py holds the property on the oracle).  So the device keeps 293
// of the 337 k-vectors, every weight doubled, and DeviceSystem::expand_S gives the reference's array
// back.  Same S, same |S|^2; the energy sums 293 terms of twice the size instead of 337.
__global__ void k_kvec_setup(double kappa, int nk, int k_sq_max, double box, int32_t *kxyz,
                             double *cfac, int16_t *kmap, int32_t *nkvecs_out, int half)
{
    const double b = 1.0 / 4.0 / kappa / kappa / box / box; // :52
    const double twopi = MMC_TWOPI, twopi_sq = twopi * twopi;
    int count = 0;
    for (int base = 0; base < 6 * 11 * 11; base += 64) {
        const int c = base + lane_id();
        const int kx = c / 121, ky = (c / 11) % 11 - 5, kz = c % 11 - 5;
        const int k_sq = kx * kx + ky * ky + kz * kz;
        const bool in_grid = c < 726 && kx <= nk && ky >= -nk && ky <= nk && kz >= -nk && kz <= nk;
        bool keep = in_grid && (k_sq < k_sq_max) && (k_sq != 0); // :76
        if (half) // (0, ky, kz) comes after (0, -ky, -kz) in this walk iff ky > 0, or ky == 0 and kz > 0
            keep = keep && !(kx == 0 && (ky > 0 || (ky == 0 && kz > 0)));
        const unsigned long long m = __ballot(keep);
        const int pos = count + lanes_below(m);
        if (keep) {
            kxyz[3 * pos] = kx; kxyz[3 * pos + 1] = ky; kxyz[3 * pos + 2] = kz;
            const double kr_sq = twopi_sq * (double)k_sq;         // :79
            double cf = twopi * exp(-b * kr_sq) / kr_sq / box;    // :80
            if (kx > 0 || half)
                cf = cf * 2.0;                                    // :81-83
            cfac[pos] = cf;
        }
        if (c < 726)
            kmap[c] = keep ? (int16_t)pos : (int16_t)-1;
        count += __popcll(m);
    }
    if (lane_id() == 0)
        *nkvecs_out = count;
}

// replica 0 -> replicas 1..R-1 (all replicas start from the same configuration)
__global__ void k_broadcast(double *base, int64_t stride, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y + 1;
    if (i < n)
        base[r * stride + i] = base[i];
}

__global__ void k_zero(double *p, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        p[i] = 0.0;
}

int32_t DeviceSystem::dmalloc(void **p, size_t bytes)
{
    MMC_HIP(hipMalloc(p, bytes ? bytes : 8));
    allocs.push_back(*p);
    return MMC_OK;
}

int32_t DeviceSystem::init(int dev, void *hip_stream, int64_t replicas)
{
    int n = 0;
    MMC_HIP(hipGetDeviceCount(&n));
    MMC_REQUIRE(n > 0, MMC_ERR_HIP, "no HIP device visible: libmmc_hip.so has no CPU fallback");
    MMC_REQUIRE(dev >= 0 && dev < n, MMC_ERR_ARG, "device %d out of range (0..%d)", dev, n - 1);
    MMC_REQUIRE(replicas >= 1, MMC_ERR_ARG, "n_replicas must be >= 1");
    device = dev;
    R = replicas;
    MMC_HIP(hipSetDevice(device));
    if (hip_stream) {
        stream = (hipStream_t)hip_stream;
        own_stream = false;
    } else {
        MMC_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        own_stream = true;
    }
    {
        int v = 0; // LDS a workgroup may have on THIS device (160 KB on MI355X, 64 KB on older parts)
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, device) == hipSuccess)
            lds_per_block = v;
    }
    MMC_HIP(hipHostMalloc(&h_res, 4096, hipHostMallocMapped));
    MMC_HIP(hipHostGetDevicePointer(&d_res, h_res, 0));
    memset(h_res, 0, 4096);
    return MMC_OK;
}

void DeviceSystem::release()
{
    (void)hipSetDevice(device);
    if (stream)
        (void)hipStreamSynchronize(stream);
    for (void *p : allocs)
        (void)hipFree(p);
    allocs.clear();
    if (h_res)
        (void)hipHostFree(h_res);
    h_res = nullptr;
    if (own_stream && stream)
        (void)hipStreamDestroy(stream);
    stream = nullptr;
}

int32_t DeviceSystem::sync()
{
    MMC_HIP(hipStreamSynchronize(stream));
    return MMC_OK;
}

int32_t DeviceSystem::upload(int64_t n_mol_, int64_t n_atoms_, const double *com,
                             const int64_t *first_atom, const int64_t *last_atom,
                             const double *coords, const int64_t *atype, const double *charge,
                             int64_t n_types_, const double *eps, const double *sig, double box_)
{
    MMC_REQUIRE(!uploaded, MMC_ERR_STATE, "system already uploaded: create a new context");
    MMC_REQUIRE(com && first_atom && last_atom && coords && atype && charge && eps && sig,
                MMC_ERR_ARG, "NULL array argument");
    MMC_REQUIRE(n_mol_ >= 1 && n_atoms_ >= 1 && n_types_ >= 1, MMC_ERR_ARG,
                "n_mol, n_atoms, n_types must be >= 1");
    MMC_REQUIRE(n_atoms_ < (1LL << 30) && n_mol_ < (1LL << 30), MMC_ERR_ARG, "system too large");
    MMC_REQUIRE(box_ > 0.0, MMC_ERR_ARG, "box must be > 0");
    MMC_REQUIRE(!ewald_ready || box_ == box, MMC_ERR_ARG,
                "system box %.17g differs from the box PrepareEwaldVariables used (%.17g)", box_,
                box);
    MMC_HIP(hipSetDevice(device));
    n_mol = n_mol_; n_atoms = n_atoms_; n_types = n_types_; box = box_;
    h_first0.resize(n_mol); h_cnt.resize(n_mol);
    uniform3 = true;
    for (int64_t j = 0; j < n_mol; j++) {
        MMC_REQUIRE(first_atom[j] >= 1 && last_atom[j] >= first_atom[j] &&
                        last_atom[j] <= n_atoms,
                    MMC_ERR_ARG, "molecule %lld: atom range [%lld, %lld] outside 1..%lld",
                    (long long)(j + 1), (long long)first_atom[j], (long long)last_atom[j],
                    (long long)n_atoms);
        h_first0[j] = (int32_t)(first_atom[j] - 1);
        h_cnt[j] = (int32_t)(last_atom[j] - first_atom[j] + 1);
        if (h_cnt[j] != 3)
            uniform3 = false;
    }
    std::vector<int32_t> h_type(n_atoms);
    for (int64_t a = 0; a < n_atoms; a++) {
        MMC_REQUIRE(atype[a] >= 1 && atype[a] <= n_types, MMC_ERR_ARG,
                    "atom %lld: type %lld outside 1..%lld", (long long)(a + 1),
                    (long long)atype[a], (long long)n_types);
        h_type[a] = (int32_t)(atype[a] - 1);
    }
    h_charge.assign(charge, charge + n_atoms);
    // homogeneous = every molecule is a copy of molecule 1 (3 atoms, same types and charges per
    // slot): what the fast per-move kernel assumes (mmc_fast.hpp)
    homogeneous = uniform3;
    for (int64_t j = 0; homogeneous && j < n_mol; j++)
        for (int t = 0; t < 3; t++)
            if (h_first0[j] != 3 * j || h_type[3 * j + t] != h_type[t] ||
                h_charge[3 * j + t] != h_charge[t])
                homogeneous = false;

    const int64_t ms = (n_mol + 15) / 16 * 16, as = (n_atoms + 15) / 16 * 16;
    bv.mol_stride = ms; bv.atom_stride = as;
    bv.n_mol = (int32_t)n_mol; bv.n_atoms = (int32_t)n_atoms; bv.n_types = (int32_t)n_types;
    bv.box = box;
    double *p;
    MMC_TRY(dmalloc((void **)&p, sizeof(double) * 3 * ms * R));
    bv.comx = p; bv.comy = p + ms * R; bv.comz = p + 2 * ms * R;
    MMC_TRY(dmalloc((void **)&p, sizeof(double) * 3 * as * R));
    bv.ax = p; bv.ay = p + as * R; bv.az = p + 2 * as * R;
    int32_t *ip;
    MMC_TRY(dmalloc((void **)&ip, sizeof(int32_t) * (2 * n_mol + n_atoms)));
    bv.first0 = ip; bv.cnt = ip + n_mol; bv.atype = ip + 2 * n_mol;
    MMC_HIP(hipMemcpy(ip, h_first0.data(), sizeof(int32_t) * n_mol, hipMemcpyHostToDevice));
    MMC_HIP(hipMemcpy(ip + n_mol, h_cnt.data(), sizeof(int32_t) * n_mol, hipMemcpyHostToDevice));
    MMC_HIP(hipMemcpy(ip + 2 * n_mol, h_type.data(), sizeof(int32_t) * n_atoms,
                      hipMemcpyHostToDevice));
    MMC_TRY(dmalloc((void **)&p, sizeof(double) * (n_atoms + 2 * n_types * n_types)));
    bv.charge = p; bv.eps = p + n_atoms; bv.sig = p + n_atoms + n_types * n_types;
    MMC_HIP(hipMemcpy(p, charge, sizeof(double) * n_atoms, hipMemcpyHostToDevice));
    MMC_HIP(hipMemcpy(p + n_atoms, eps, sizeof(double) * n_types * n_types,
                      hipMemcpyHostToDevice));
    MMC_HIP(hipMemcpy(p + n_atoms + n_types * n_types, sig, sizeof(double) * n_types * n_types,
                      hipMemcpyHostToDevice));
    if (homogeneous) {
        MMC_TRY(dmalloc((void **)&rec, sizeof(double) * MMC_RSTRIDE * n_mol * R));
        MMC_HIP(hipMemset(rec, 0, sizeof(double) * MMC_RSTRIDE * n_mol * R));
        bv.cq_stride = (n_mol + 63) / 64 * 64;
        // (+ MMC_CQ_PAD bytes: the COM scan of the wave kernels prefetches unclamped past the end)
        MMC_TRY(dmalloc((void **)&bv.comq, sizeof(uint16_t) * 3 * bv.cq_stride * R + MMC_CQ_PAD));
        MMC_HIP(hipMemset(bv.comq, 0, sizeof(uint16_t) * 3 * bv.cq_stride * R + MMC_CQ_PAD));
        memset(&fc, 0, sizeof(fc)); // launch constants of the fast kernels
        for (int ab = 0; ab < 9; ab++) {
            const int a = ab / 3, c = ab % 3;
            const int64_t ta = h_type[a], tb = h_type[c];
            fc.qq9[ab] = charge[a] * charge[c];
            if (fc.qq9[ab] < 0)
                fc.qneg_mask |= 1 << ab;
            const double e = eps[ta + tb * n_types];
            fc.eps9[ab] = e;
            fc.sig9[ab] = sig[ta + tb * n_types];
            if (e > 0.001) { // energy.jl:270
                fc.lj_mask |= 1 << ab;
                fc.ljp_ab[fc.n_ljp] = ab;
                fc.ljp_eps[fc.n_ljp] = e;
                fc.ljp_sig[fc.n_ljp] = sig[ta + tb * n_types];
                fc.n_ljp++;
            }
        }
        for (int a = 0; a < 3; a++)
            fc.q[a] = charge[a];
        const int nt = (int)((n_mol + MMC_TM - 1) / MMC_TM); // tile pairs I <= J of k_total_pairs
        std::vector<int16_t> tp;
        for (int i = 0; i < nt; i++)
            for (int j = i; j < nt; j++) {
                tp.push_back((int16_t)i);
                tp.push_back((int16_t)j);
            }
        n_tile_pairs = (int)(tp.size() / 2);
        MMC_REQUIRE(nt < 32768, MMC_ERR_UNSUPPORTED, "too many molecule tiles");
        MMC_TRY(dmalloc((void **)&tile_pairs, sizeof(int16_t) * tp.size()));
        MMC_HIP(hipMemcpy(tile_pairs, tp.data(), sizeof(int16_t) * tp.size(),
                          hipMemcpyHostToDevice));
    }
    MMC_TRY(dmalloc((void **)&d_permol, sizeof(MolE) * n_mol * R));
    MMC_TRY(dmalloc(&d_scr, 64 * (size_t)R)); // per-replica result scratch (TotalsRaw / double)
    MMC_TRY(dmalloc((void **)&d_stage, sizeof(double) * 3 * (n_atoms + n_mol)));
    h_stage.resize(3 * (n_atoms + n_mol));
    uploaded = true;
    MMC_TRY(set_replica(0, com, coords));
    if (R > 1)
        MMC_TRY(broadcast_replica0());
    return MMC_OK;
}

void DeviceSystem::note_shape(const double *com, const double *coords)
{
    if (!com || !coords) { // atoms without their centres of mass: nothing is known any more
        r_mol_max = INFINITY;
        return;
    }
    double m2 = 0.0;
    for (int64_t j = 0; j < n_mol; j++)
        for (int64_t a = h_first0[j]; a < h_first0[j] + h_cnt[j]; a++) {
            const double dx = coords[3 * a] - com[3 * j], dy = coords[3 * a + 1] - com[3 * j + 1],
                         dz = coords[3 * a + 2] - com[3 * j + 2];
            m2 = std::max(m2, dx * dx + dy * dy + dz * dz);
        }
    r_mol_max = std::max(r_mol_max, std::sqrt(m2));
}

// gate + 2 r_mol < box / 2, with room for the rounding of millions of rigid moves
bool DeviceSystem::image_by_molecule(double gate_sq) const
{
    return std::isfinite(r_mol_max) && std::sqrt(gate_sq) + 2.0 * r_mol_max + 1e-6 < 0.5 * box;
}
// ... and every atom pair of a gated molecule pair lies inside the slack r_cut^2 + 100 of
// ewalds.jl:362 / energy.jl:270 (for water, r_mol < 1 A: whenever r_cut < 24 A)
bool DeviceSystem::pairs_inside_slack(double gate_sq, double slack_sq) const
{
    const double far = std::sqrt(gate_sq) + 2.0 * r_mol_max + 1e-6;
    return std::isfinite(r_mol_max) && far * far < slack_sq;
}

int32_t DeviceSystem::set_replica(int64_t r, const double *com, const double *coords)
{
    MMC_REQUIRE(uploaded, MMC_ERR_STATE, "no system uploaded");
    MMC_REQUIRE(r >= 0 && r < R, MMC_ERR_ARG, "replica %lld outside 0..%lld", (long long)r,
                (long long)(R - 1));
    MMC_REQUIRE(coords, MMC_ERR_ARG, "NULL array argument");
    MMC_HIP(hipSetDevice(device));
    MMC_HIP(hipMemcpyAsync(d_stage, coords, sizeof(double) * 3 * n_atoms, hipMemcpyHostToDevice,
                           stream));
    k_aos_to_soa<<<(n_atoms + 255) / 256, 256, 0, stream>>>(
        d_stage, bv.ax + r * bv.atom_stride, bv.ay + r * bv.atom_stride,
        bv.az + r * bv.atom_stride, (int)n_atoms);
    if (com) { // com == NULL: atoms only (RecipLong reads nothing else)
        MMC_HIP(hipMemcpyAsync(d_stage + 3 * n_atoms, com, sizeof(double) * 3 * n_mol,
                               hipMemcpyHostToDevice, stream));
        k_aos_to_soa<<<(n_mol + 255) / 256, 256, 0, stream>>>(
            d_stage + 3 * n_atoms, bv.comx + r * bv.mol_stride, bv.comy + r * bv.mol_stride,
            bv.comz + r * bv.mol_stride, (int)n_mol);
    }
    if (rec)
        k_build_rec<<<(n_mol + 255) / 256, 256, 0, stream>>>(bv, rec, (int)r);
    comq_epoch++;
    MMC_HIP(hipGetLastError());
    note_shape(com, coords);
    return sync(); // the host arrays are borrowed for the call only
}

int32_t DeviceSystem::get_replica(int64_t r, double *com, double *coords)
{
    MMC_REQUIRE(uploaded, MMC_ERR_STATE, "no system uploaded");
    MMC_REQUIRE(r >= 0 && r < R, MMC_ERR_ARG, "replica %lld outside 0..%lld", (long long)r,
                (long long)(R - 1));
    MMC_HIP(hipSetDevice(device));
    k_soa_to_aos<<<(n_atoms + 255) / 256, 256, 0, stream>>>(
        bv.ax + r * bv.atom_stride, bv.ay + r * bv.atom_stride, bv.az + r * bv.atom_stride,
        d_stage, (int)n_atoms);
    k_soa_to_aos<<<(n_mol + 255) / 256, 256, 0, stream>>>(
        bv.comx + r * bv.mol_stride, bv.comy + r * bv.mol_stride, bv.comz + r * bv.mol_stride,
        d_stage + 3 * n_atoms, (int)n_mol);
    MMC_HIP(hipGetLastError());
    if (coords)
        MMC_HIP(hipMemcpyAsync(coords, d_stage, sizeof(double) * 3 * n_atoms,
                               hipMemcpyDeviceToHost, stream));
    if (com)
        MMC_HIP(hipMemcpyAsync(com, d_stage + 3 * n_atoms, sizeof(double) * 3 * n_mol,
                               hipMemcpyDeviceToHost, stream));
    return sync();
}

int32_t DeviceSystem::broadcast_replica0()
{
    if (R <= 1)
        return MMC_OK;
    dim3 ga((unsigned)((n_atoms + 255) / 256), (unsigned)(R - 1));
    dim3 gm((unsigned)((n_mol + 255) / 256), (unsigned)(R - 1));
    k_broadcast<<<ga, 256, 0, stream>>>(bv.ax, bv.atom_stride, (int)n_atoms);
    k_broadcast<<<ga, 256, 0, stream>>>(bv.ay, bv.atom_stride, (int)n_atoms);
    k_broadcast<<<ga, 256, 0, stream>>>(bv.az, bv.atom_stride, (int)n_atoms);
    k_broadcast<<<gm, 256, 0, stream>>>(bv.comx, bv.mol_stride, (int)n_mol);
    k_broadcast<<<gm, 256, 0, stream>>>(bv.comy, bv.mol_stride, (int)n_mol);
    k_broadcast<<<gm, 256, 0, stream>>>(bv.comz, bv.mol_stride, (int)n_mol);
    if (rec) {
        const int64_t per = MMC_RSTRIDE * n_mol;
        dim3 gr((unsigned)((per + 255) / 256), (unsigned)(R - 1));
        k_broadcast_rec<<<gr, 256, 0, stream>>>(rec, per);
        const int64_t perf = 3 * bv.cq_stride / 2; // the 16-bit codes, two to a 32-bit word
        dim3 gf((unsigned)((perf + 255) / 256), (unsigned)(R - 1));
        k_broadcast_f32<<<gf, 256, 0, stream>>>(reinterpret_cast<float *>(bv.comq), perf);
        comq_epoch++;
    }
    MMC_HIP(hipGetLastError());
    return sync();
}

int32_t DeviceSystem::prepare_ewald(double kappa, int64_t nk_, int64_t k_sq_max_, double box_,
                                    double factor, int64_t *nkvecs_out)
{
    MMC_REQUIRE(k_sq_max_ == 27, MMC_ERR_ASSERT, "AssertionError: k_sq_max == 27 (ewalds.jl:49)");
    MMC_REQUIRE(nk_ >= 0 && kappa > 0.0 && box_ > 0.0, MMC_ERR_ARG, "bad kappa/nk/box");
    MMC_HIP(hipSetDevice(device));
    if (uploaded)
        MMC_REQUIRE(box_ == box, MMC_ERR_ARG,
                    "PrepareEwaldVariables box %.17g differs from the uploaded system's %.17g",
                    box_, box);
    else
        bv.box = box = box_;
    if (!bv.S) {
        double *p;
        // (a context, R = 1, names four buffers: old, new, a speculative sum, a spare -- mmc_ctx.inc)
        MMC_TRY(dmalloc((void **)&p, sizeof(double) * 2 * (R == 1 ? 4 : 2) * MMC_NK_STRIDE * R));
        bv.S = p;
        bv.nk_stride = MMC_NK_STRIDE;
        int32_t *ip;
        MMC_TRY(dmalloc((void **)&ip, sizeof(int32_t) * 3 * MMC_NK_STRIDE));
        bv.kxyz = ip;
        MMC_TRY(dmalloc((void **)&p, sizeof(double) * MMC_NK_STRIDE));
        bv.cfac = p;
        int16_t *sp;
        MMC_TRY(dmalloc((void **)&sp, sizeof(int16_t) * 6 * 11 * 11));
        bv.kmap = sp;
    }
    k_kvec_setup<<<1, 64, 0, stream>>>(kappa, (int)(nk_ > 5 ? 5 : nk_), (int)k_sq_max_, box_,
                                       (int32_t *)bv.kxyz, (double *)bv.cfac,
                                       (int16_t *)bv.kmap, (int32_t *)d_res, half_k ? 1 : 0);
    if (!qq_tab)
        MMC_TRY(dmalloc((void **)&qq_tab, sizeof(double) * MMC_QQ_TABLE_DOUBLES));
    k_build_qq_table<<<(MMC_QQ_NROW + 63) / 64, 64, 0, stream>>>(kappa, qq_tab);
    if (!kpack)
        MMC_TRY(dmalloc((void **)&kpack, sizeof(int32_t) * (MMC_NK_STRIDE + MMC_KCOLS)));
    k_pack_kvec<<<1, MMC_NK_STRIDE, 0, stream>>>(bv.kxyz, (const int32_t *)d_res, kpack);
    const int64_t ns = 2 * (R == 1 ? 4 : 2) * MMC_NK_STRIDE * R; // zeros(ComplexF64, NKVECS) x2 (:98-99)
    k_zero<<<(unsigned)((ns + 255) / 256), 256, 0, stream>>>(bv.S, ns);
    MMC_HIP(hipGetLastError());
    MMC_TRY(sync());
    nkvecs = *(volatile int32_t *)h_res;
    nk = nk_; k_sq_max = k_sq_max_;
    { // the reference's list (ewalds.jl:57-89 order) -> the device's: index, or ~index of the conjugate
        const int nkc = (int)(nk_ > 5 ? 5 : nk_);
        int16_t dev_of[6 * 11 * 11];
        ref_to_dev.clear();
        int n_dev = 0;
        for (int kx = 0; kx <= nkc; kx++)
            for (int ky = -nkc; ky <= nkc; ky++)
                for (int kz = -nkc; kz <= nkc; kz++) {
                    const int k2 = kx * kx + ky * ky + kz * kz;
                    if (k2 == 0 || k2 >= (int)k_sq_max_)
                        continue;
                    const bool later = half_k && kx == 0 && (ky > 0 || (ky == 0 && kz > 0));
                    if (later)
                        ref_to_dev.push_back(~(int32_t)dev_of[((5 - ky) * 11) + (5 - kz)]);
                    else {
                        dev_of[(kx * 11 + ky + 5) * 11 + kz + 5] = (int16_t)n_dev;
                        ref_to_dev.push_back(n_dev++);
                    }
                }
        nkvecs_ref = (int64_t)ref_to_dev.size();
        MMC_REQUIRE(n_dev == nkvecs, MMC_ERR_ASSERT, "k-vector walk: host %d, device %d", n_dev, (int)nkvecs);
    }
    bv.nkvecs = (int32_t)nkvecs; bv.nk = (int32_t)nk_;
    bv.kappa = kappa; bv.factor = factor;
    { // work queue of k_recip_long_lds: the columns that hold a k-vector (ewalds.jl:57-66), in
      // descending order of complex products per atom (powers of x and y, the z recurrence, kz terms)
        struct Col { int c, cost; };
        std::vector<Col> cols;
        const int nkc = (int)(nk_ > 5 ? 5 : nk_);
        for (int kx = 0; kx <= nkc; kx++)
            for (int ky = -nkc; ky <= nkc; ky++) {
                int m = -1;
                for (int kz = 0; kz <= nkc; kz++) {
                    const int k2 = kx * kx + ky * ky + kz * kz;
                    if (k2 > 0 && k2 < (int)k_sq_max_)
                        m = kz;
                }
                if (m < 0 || (half_k && kx == 0 && ky > 0)) // (a column of conjugates only: not kept)
                    continue;
                const int aky = ky < 0 ? -ky : ky, mm = m < 1 ? 1 : m;
                cols.push_back({ kx * MMC_NKTAB + ky + 5,
                                 (kx > 1 ? kx - 1 : 0) + (aky > 1 ? aky - 1 : 0) + (mm - 1) + 2 + (2 * mm + 1) });
            }
        std::stable_sort(cols.begin(), cols.end(), [](const Col &a, const Col &b) { return a.cost > b.cost; });
        memset(&recip_order, 0, sizeof(recip_order));
        recip_order.n = (int32_t)cols.size();
        for (size_t k = 0; k < cols.size(); k++)
            recip_order.col[k] = (uint8_t)cols[k].c;
    }
    ewald_ready = true;
    if (nkvecs_out)
        *nkvecs_out = nkvecs_ref;
    return MMC_OK;
}

// device order (bv.nkvecs complex numbers) -> the reference's sumQExp array (nkvecs_ref of them)
void DeviceSystem::expand_S(const double *dev_order, double *ref_order) const
{
    for (size_t k = 0; k < ref_to_dev.size(); k++) {
        const int32_t d = ref_to_dev[k];
        if (d >= 0) {
            ref_order[2 * k] = dev_order[2 * d];
            ref_order[2 * k + 1] = dev_order[2 * d + 1];
        } else {
            ref_order[2 * k] = dev_order[2 * (~d)];
            ref_order[2 * k + 1] = -dev_order[2 * (~d) + 1];
        }
    }
}

PairParams mmc_pair_params(double lj_rcut, double qq_rcut, double diameter, double ovr,
                           double kappa, bool bare)
{
    PairParams pp;
    const double lg = lj_rcut + diameter, qg = qq_rcut + diameter;
    pp.lj_gate_sq = lg * lg;                 // energy.jl:233-234
    pp.qq_gate_sq = qg * qg;                 // ewalds.jl:313-314
    pp.lj_slack_sq = lj_rcut * lj_rcut + 100; // energy.jl:270
    pp.qq_slack_sq = bare ? qq_rcut * qq_rcut : qq_rcut * qq_rcut + 100; // energy.jl:699 / ewalds.jl:362
    pp.ovr = ovr;
    pp.kappa = kappa;
    return pp;
}

int32_t DeviceSystem::mol_energy(int i_base, int n_sel, bool lj, bool qq, int style,
                                 const PairParams &pp, MolE *out, int out_stride)
{
    dim3 grid((unsigned)n_sel, (unsigned)R);
    if (lj && qq && style == 0)
        k_mol_energy<true, true, 0><<<grid, MMC_BLOCK, 0, stream>>>(bv, i_base, pp, out, out_stride);
    else if (lj && !qq)
        k_mol_energy<true, false, 0><<<grid, MMC_BLOCK, 0, stream>>>(bv, i_base, pp, out, out_stride);
    else if (!lj && qq && style == 0)
        k_mol_energy<false, true, 0><<<grid, MMC_BLOCK, 0, stream>>>(bv, i_base, pp, out, out_stride);
    else if (!lj && qq && style == 1)
        k_mol_energy<false, true, 1><<<grid, MMC_BLOCK, 0, stream>>>(bv, i_base, pp, out, out_stride);
    else {
        mmc_set_error("unsupported term combination");
        return MMC_ERR_UNSUPPORTED;
    }
    MMC_HIP(hipGetLastError());
    return MMC_OK;
}

int32_t DeviceSystem::recip_long_all(double *energies_host)
{
    if (R == 1 && uploaded && ewald_ready && nk == 5 && !pb.on) { // one system: one launch, no copy
        PotOneOut o;
        MMC_TRY(potential_one(0.0, 0.0, false, true, &o));
        energies_host[0] = o.recip_e;
        return MMC_OK;
    }
    MMC_TRY(recip_long_enqueue(energies_host));
    return sync();
}

// One system in one launch (k_potential_one): the pair totals of potential() (homogeneous systems
// the erfc table covers) and / or the structure factor with its energy.  Results arrive in pinned
// host memory behind a stamp; the host polls it.
int32_t DeviceSystem::potential_one(double lj_rcut, double qq_rcut, bool pairs, bool recip,
                                    PotOneOut *res)
{
    MMC_REQUIRE(R == 1 && uploaded && ewald_ready, MMC_ERR_STATE, "potential_one: one prepared system");
    MMC_HIP(hipSetDevice(device));
    PotOneArgs a;
    memset(&a, 0, sizeof(a));
    if (!d_ticket) {
        MMC_TRY(dmalloc((void **)&d_ticket, 512));
        MMC_HIP(hipMemsetAsync(d_ticket, 0, 512, stream));
        MMC_TRY(dmalloc((void **)&d_spart1, sizeof(double) * 2 * MMC_NK_STRIDE * POT_MAX_CHUNKS));
    }
    PairParams pp = mmc_pair_params(1.0, 1.0, 0.0, 0.5, bv.kappa, false);
    if (pairs) {
        MMC_REQUIRE(fast_table_ok(qq_rcut), MMC_ERR_UNSUPPORTED, "potential_one: no pair fast path");
        pp = mmc_pair_params(lj_rcut, qq_rcut, 0.0, 0.5, bv.kappa, false);
        // units of (molecule, j-range of POT_JCHUNK molecules) while that stays a few thousand waves
        // (measured at 750 molecules: every additional 100 workgroups cost ~1 us -- table copy,
        // ticket -- so rows are split only on request)
        const int jc = getenv("MMC_POT_JCHUNK") ? atoi(getenv("MMC_POT_JCHUNK")) : 0;
        const int64_t n_ch = jc > 0 ? (n_mol + jc - 1) / jc : 1;
        if (!d_tparts1)
            MMC_TRY(dmalloc((void **)&d_tparts1, sizeof(TotalPart) * (size_t)(n_mol * n_ch)));
        a.tparts = d_tparts1;
        a.j_chunk = n_ch > 1 ? jc : 0;
        a.n_units = (int)(n_mol * n_ch);
        a.pair_wgs = (int)((a.n_units + WV_WAVES - 1) / WV_WAVES);
    }
    if (recip) {
        const int per = getenv("MMC_POT_CHUNK") ? atoi(getenv("MMC_POT_CHUNK")) : POT_CHUNK_ATOMS;
        int n_chunks = (int)((n_atoms + per - 1) / per);
        if (n_chunks > POT_MAX_CHUNKS) n_chunks = POT_MAX_CHUNKS;
        int chunk_len = (int)((n_atoms + n_chunks - 1) / n_chunks);
        chunk_len = (chunk_len + MMC_BLOCK - 1) / MMC_BLOCK * MMC_BLOCK;
        n_chunks = (int)((n_atoms + chunk_len - 1) / chunk_len);
        a.spart = d_spart1;
        a.n_cols = recip_order.n;
        a.n_chunks = n_chunks;
        a.chunk_len = chunk_len;
    }
    a.counter = d_ticket;
    PotOneOut *h_out = reinterpret_cast<PotOneOut *>((char *)h_res + 1024);
    a.out = reinterpret_cast<PotOneOut *>((char *)d_res + 1024);
    a.stamp = ++pot_stamp ? pot_stamp : ++pot_stamp; // never 0
    const unsigned grid = (unsigned)(a.pair_wgs + a.n_cols * a.n_chunks);
    MMC_REQUIRE(grid > 0, MMC_ERR_ARG, "potential_one: nothing to do");
    if (image_by_molecule(std::max(pp.lj_gate_sq, pp.qq_gate_sq)) && pairs_inside_slack(pp.qq_gate_sq, pp.qq_slack_sq)
        && pairs_inside_slack(pp.lj_gate_sq, pp.lj_slack_sq))
        k_potential_one<true><<<grid, MMC_BLOCK, 0, stream>>>(bv, rec, qq_tab, fc, pp, recip_order, a);
    else
        k_potential_one<false><<<grid, MMC_BLOCK, 0, stream>>>(bv, rec, qq_tab, fc, pp, recip_order, a);
    MMC_HIP(hipGetLastError());
    const volatile uint32_t *st = &h_out->stamp;
    for (unsigned spins = 1; *st != a.stamp; spins++) {
        if ((spins & 0xfff) == 0) {
            const hipError_t q = hipStreamQuery(stream);
            if (q == hipSuccess) { // the kernel has ended: its last store is on its way
                MMC_HIP(hipStreamSynchronize(stream));
                MMC_REQUIRE(*st == a.stamp, MMC_ERR_HIP, "k_potential_one ended without posting its result");
                break;
            }
            MMC_REQUIRE(q == hipErrorNotReady, MMC_ERR_HIP, "k_potential_one failed: %s",
                        hipGetErrorString(q));
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    memcpy(res, (const void *)h_out, sizeof(PotOneOut));
    return MMC_OK;
}

// RecipLong for every replica, enqueued on the stream without waiting: the energies land in
// `energies_host` (pinned or pageable) once the stream has been synchronised.
int32_t DeviceSystem::recip_long_enqueue(double *energies_host)
{
    MMC_REQUIRE(uploaded && ewald_ready, MMC_ERR_STATE,
                "RecipLong needs an uploaded system and PrepareEwaldVariables");
    MMC_HIP(hipSetDevice(device));
    double *d_e = (double *)d_scr;
    dim3 grid(6 * MMC_NKTAB, (unsigned)R);
    // 3 sincos per atom once (k_atom_phases) instead of once per (kx, ky) column; the scratch is
    // 48 B per atom and replica, so very large batches keep the recomputing kernel
    // many replicas of a system whose phases fit a compute unit's LDS: one workgroup per replica
    // (the kernel has 8 bytes of static LDS besides; what the device grants is asked of the
    // device, and a refusal falls through to the column kernels below)
    const size_t lds_bytes = sizeof(double) * 7 * (size_t)n_atoms;
    // (per-replica boxes: always the phase path below, its two box-dependent kernels per box)
    if (!pb.on && 66 * R >= 16384 && (int64_t)lds_bytes + 64 <= lds_per_block && !recip_lds_refused
        && !getenv("MMC_NO_RECIP_LDS")) {
        if (!recip_lds_ready) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_recip_long_lds),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)(lds_per_block - 64));
            if (e != hipSuccess) {
                (void)hipGetLastError();
                recip_lds_refused = true;
            } else {
                recip_lds_ready = true;
            }
        }
    }
    if (!pb.on && 66 * R >= 16384 && (int64_t)lds_bytes + 64 <= lds_per_block && recip_lds_ready
        && !getenv("MMC_NO_RECIP_LDS")) {
        k_recip_long_lds<<<(unsigned)R, RL_WAVES * 64, lds_bytes, stream>>>(bv, recip_order);
        k_recip_energy<<<(unsigned)R, MMC_BLOCK, 0, stream>>>(bv, 1, d_e);
        MMC_HIP(hipGetLastError());
        MMC_HIP(hipMemcpyAsync(energies_host, d_e, sizeof(double) * R, hipMemcpyDeviceToHost,
                               stream));
        return MMC_OK;
    }
    const size_t ph_bytes = sizeof(double) * 6 * (size_t)n_atoms * (size_t)R;
    if (!d_phase && ph_bytes <= ((size_t)8 << 30))
        MMC_TRY(dmalloc((void **)&d_phase, ph_bytes));
    MMC_REQUIRE(d_phase || !pb.on, MMC_ERR_UNSUPPORTED,
                "per-replica boxes: %lld replicas of %lld atoms are too many for the phase array",
                (long long)R, (long long)n_atoms);
    if (d_phase) {
        dim3 ga((unsigned)((n_atoms + 255) / 256), (unsigned)R);
        if (pb.on)
            k_atom_phases_pb<<<ga, 256, 0, stream>>>(bv, d_phase, pb.d_box);
        else
            k_atom_phases<<<ga, 256, 0, stream>>>(bv, d_phase);
        // few replicas: split the atoms over up to 16 chunks so that the chip is busy
        int n_chunks = 1;
        if (66 * R < 1024) {
            n_chunks = (int)std::min<int64_t>((n_atoms + MMC_BLOCK - 1) / MMC_BLOCK,
                                              std::min<int64_t>(16, 1024 / (66 * R)));
            if (n_chunks < 1) n_chunks = 1;
        }
        int chunk_len = (int)((n_atoms + n_chunks - 1) / n_chunks);
        chunk_len = (chunk_len + MMC_BLOCK - 1) / MMC_BLOCK * MMC_BLOCK;
        n_chunks = (int)((n_atoms + chunk_len - 1) / chunk_len);
        if (n_chunks > 1 && !d_spart)
            MMC_TRY(dmalloc((void **)&d_spart, sizeof(double) * 2 * MMC_NK_STRIDE * 16 * (size_t)R));
        dim3 gridc(6 * MMC_NKTAB, (unsigned)R, (unsigned)n_chunks);
        if (n_chunks == 1 && 66 * R >= 16384) // many replicas: a wave per column
            k_recip_long_ph<64><<<gridc, 64, 0, stream>>>(bv, d_phase, d_spart, chunk_len);
        else
            k_recip_long_ph<MMC_BLOCK><<<gridc, MMC_BLOCK, 0, stream>>>(bv, d_phase, d_spart, chunk_len);
        if (n_chunks > 1) {
            dim3 gf((unsigned)((2 * nkvecs + 255) / 256), (unsigned)R);
            k_recip_finish<<<gf, 256, 0, stream>>>(bv, d_spart, n_chunks);
        }
    } else {
        k_recip_long<<<grid, MMC_BLOCK, 0, stream>>>(bv);
    }
    if (pb.on)
        k_recip_energy_pb<<<(unsigned)R, MMC_BLOCK, 0, stream>>>(bv, 1, d_e, pb.cfac);
    else
        k_recip_energy<<<(unsigned)R, MMC_BLOCK, 0, stream>>>(bv, 1, d_e);
    MMC_HIP(hipGetLastError());
    MMC_HIP(hipMemcpyAsync(energies_host, d_e, sizeof(double) * R, hipMemcpyDeviceToHost,
                           stream));
    return MMC_OK;
}

int32_t DeviceSystem::charge_sums(double *sum_q, double *sum_q2)
{
    if (sums_valid) { // the charges are fixed at upload
        *sum_q = c_sq;
        *sum_q2 = c_sq2;
        return MMC_OK;
    }
    MMC_HIP(hipSetDevice(device));
    k_charge_sums<<<1, MMC_BLOCK, 0, stream>>>(bv.charge, (int)n_atoms, (double *)d_res);
    MMC_HIP(hipGetLastError());
    MMC_TRY(sync());
    *sum_q = c_sq = ((volatile double *)h_res)[0];
    *sum_q2 = c_sq2 = ((volatile double *)h_res)[1];
    sums_valid = true;
    return MMC_OK;
}

// The erfc(kappa r)/r table spans r^2 in [0.25, UMAX), is accurate for kappa*r <= XMAX, and its
// small-r series needs kappa * 0.5 A <= 0.25 (mmc_fast.hpp).
bool DeviceSystem::fast_table_ok(double qq_rcut) const
{
    const double slack = qq_rcut * qq_rcut + 100; // ewalds.jl:362
    return homogeneous && rec && ewald_ready && bv.kappa <= MMC_QQ_KAPPA_MAX &&
           slack <= MMC_QQ_UMAX && bv.kappa * std::sqrt(slack) <= MMC_QQ_XMAX;
}

// The two per-molecule loops of potential() (energy.jl:972-977, :991-1000) for every replica.
// Homogeneous systems: every molecule pair once (k_total_pairs); a replica in which any atom pair
// overlaps, and every other kind of system, goes through the per-molecule kernels, which
// reproduce the reference loop literally (each pair twice, EwaldReal = 0 for an overlapping
// molecule).
int32_t DeviceSystem::pair_totals(double lj_rcut, double qq_rcut, std::vector<TotalsRaw> &ht)
{
    bool fast = false;
    MMC_TRY(pair_totals_enqueue(lj_rcut, qq_rcut, ht, &fast));
    if (fast)
        MMC_TRY(sync());
    return pair_totals_finish(lj_rcut, qq_rcut, ht, fast);
}

// Enqueue the half-pair kernels (homogeneous systems) and the copy of their results into `ht`
// without waiting; *fast says whether anything was enqueued.
int32_t DeviceSystem::pair_totals_enqueue(double lj_rcut, double qq_rcut,
                                          std::vector<TotalsRaw> &ht, bool *fast)
{
    const PairParams pp = mmc_pair_params(lj_rcut, qq_rcut, 0.0, 0.5, bv.kappa, false);
    ht.resize(R);
    TotalsRaw *d_t = (TotalsRaw *)d_scr;
    *fast = pb.on || fast_table_ok(qq_rcut); // (mmc_batch_set_boxes checked the table's domain)
    if (!*fast)
        return MMC_OK;
    // k_total_wave: a wave per pair of molecules (u, n_mol - 1 - u), see mmc_wave.hpp
    const int paired = (n_mol + 1) / 2 * R >= 4096 ? 1 : 0; // enough waves to fill the chip?
    const int units = paired ? (int)((n_mol + 1) / 2) : (int)n_mol;
    if (!d_tparts)
        MMC_TRY(dmalloc((void **)&d_tparts, sizeof(TotalPart) * (size_t)n_mol * R));
    const int64_t n_units = (int64_t)units * R;
    MMC_REQUIRE(n_units < (1LL << 31), MMC_ERR_UNSUPPORTED, "too many (replica, molecule) units");
    // One unit per wave, NOT persistent: the ~375 units of a replica share its 105 KB of
    // records, and only in-order dispatch keeps the units in flight within a few replicas of
    // each other.  (Persistent waves striding through the units drift apart by hundreds of
    // replicas, the working set outgrows the 4 MB L2s and the hit rate drops to 46 %: measured,
    // 5.2 MB of fabric traffic per evaluation instead of ~1.)
    const int64_t wgs = (n_units + WV_WAVES - 1) / WV_WAVES;
    if (pb.on) {
        // per-replica boxes: k_total_wave once per replica, on a view in which replica r is
        // replica 0 with its own box, kappa and table (the prefilter codes first: the commit
        // kernels of the move driver write them as fractions of bv.box)
        dim3 gq((unsigned)((n_mol + 255) / 256), (unsigned)R);
        k_comq_pb<<<gq, 256, 0, stream>>>(bv, pb.d_box);
        comq_epoch++;
        const int64_t wgs1 = (units + WV_WAVES - 1) / WV_WAVES;
        for (int64_t r = 0; r < R; r++) {
            BatchView v = bv;
            v.comx += r * bv.mol_stride; v.comy += r * bv.mol_stride; v.comz += r * bv.mol_stride;
            v.ax += r * bv.atom_stride; v.ay += r * bv.atom_stride; v.az += r * bv.atom_stride;
            v.comq += r * 3 * bv.cq_stride;
            v.box = pb.box[r];
            v.kappa = pb.kappa[r];
            const PairParams ppr = mmc_pair_params(lj_rcut, qq_rcut, 0.0, 0.5, pb.kappa[r], false);
            k_total_wave<false><<<(unsigned)wgs1, WV_WAVES * 64, 0, stream>>>(
                v, rec + r * n_mol * MMC_RSTRIDE, pb.tab + r * MMC_QQ_TABLE_DOUBLES, fc, ppr,
                d_tparts + r * units, units, units, paired);
        }
    } else if (image_by_molecule(std::max(pp.lj_gate_sq, pp.qq_gate_sq)) && pairs_inside_slack(pp.qq_gate_sq, pp.qq_slack_sq)
        && pairs_inside_slack(pp.lj_gate_sq, pp.lj_slack_sq))
        k_total_wave<true><<<(unsigned)wgs, WV_WAVES * 64, 0, stream>>>(bv, rec, qq_tab, fc, pp, d_tparts,
                                                                        units, (int)n_units, paired);
    else
        k_total_wave<false><<<(unsigned)wgs, WV_WAVES * 64, 0, stream>>>(bv, rec, qq_tab, fc, pp, d_tparts,
                                                                         units, (int)n_units, paired);
    k_total_reduce<<<(unsigned)R, MMC_BLOCK, 0, stream>>>(d_tparts, units, d_t);
    MMC_HIP(hipGetLastError());
    MMC_HIP(hipMemcpyAsync(ht.data(), d_t, sizeof(TotalsRaw) * R, hipMemcpyDeviceToHost, stream));
    return MMC_OK;
}

// After the stream has been synchronised: a replica in which any atom pair overlaps, and every
// other kind of system, goes through the per-molecule kernels, which reproduce the reference loop
// literally (each pair twice, EwaldReal = 0 for an overlapping molecule).
int32_t DeviceSystem::pair_totals_finish(double lj_rcut, double qq_rcut,
                                         std::vector<TotalsRaw> &ht, bool fast)
{
    bool need_generic = !fast;
    for (int64_t r = 0; fast && r < R; r++)
        if (ht[r].n_ovl)
            need_generic = true; // overlap sentinel
    if (pb.on) { // (the per-molecule kernels know one box: totals_ewald reports the overlap)
        MMC_REQUIRE(fast, MMC_ERR_UNSUPPORTED, "per-replica boxes need the erfc table's fast path");
        return MMC_OK;
    }
    if (need_generic) {
        const PairParams pp = mmc_pair_params(lj_rcut, qq_rcut, 0.0, 0.5, bv.kappa, false);
        TotalsRaw *d_t = (TotalsRaw *)d_scr;
        MMC_TRY(mol_energy(0, (int)n_mol, true, true, 0, pp, d_permol, (int)n_mol));
        k_totals<<<(unsigned)R, MMC_BLOCK, 0, stream>>>(d_permol, (int)n_mol, (int)n_mol, d_t);
        MMC_HIP(hipGetLastError());
        MMC_HIP(hipMemcpyAsync(ht.data(), d_t, sizeof(TotalsRaw) * R, hipMemcpyDeviceToHost,
                               stream));
        MMC_TRY(sync());
    }
    return MMC_OK;
}

// The coordinate and table part of an NPT volume move (volumeChange.jl:59-80 is the reference's
// only specification: text in a docstring): COMs scale by L_new/L_old, atoms follow rigidly, and
// everything that depends on the box is rebuilt -- kappa = alpha/L_new, kxyz/cfac
// (PrepareEwaldVariables, ewalds.jl:45-103), the erfc table.  The total energy at the new volume is
// then one totals_ewald() call (K2 + K3).
int32_t DeviceSystem::volume_change(double new_box, double new_kappa)
{
    MMC_REQUIRE(uploaded && ewald_ready, MMC_ERR_STATE,
                "volume change needs an uploaded system and PrepareEwaldVariables");
    MMC_REQUIRE(new_box > 0.0 && new_kappa > 0.0, MMC_ERR_ARG, "bad box/kappa");
    MMC_HIP(hipSetDevice(device));
    const double f = new_box / box;
    dim3 grid((unsigned)((n_mol + 255) / 256), (unsigned)R);
    BatchView nbv = bv;
    nbv.box = new_box; // the fixed-point centres of mass are fractions of the NEW box
    k_rescale<<<grid, 256, 0, stream>>>(nbv, rec, f);
    comq_epoch++; // (and the prefilter's threshold changes with the box)
    MMC_HIP(hipGetLastError());
    box = bv.box = new_box;
    return prepare_ewald(new_kappa, nk, k_sq_max, new_box, bv.factor, nullptr);
}

int32_t DeviceSystem::snapshot_take()
{
    MMC_REQUIRE(uploaded && ewald_ready, MMC_ERR_STATE, "snapshot: no prepared system");
    MMC_HIP(hipSetDevice(device));
    if (!snap.buf) {
        struct Seg { const void *p; int64_t bytes; };
        const int nsb = R == 1 ? 4 : 2;
        const Seg segs[] = {
            { bv.comx, (int64_t)sizeof(double) * 3 * bv.mol_stride * R },
            { bv.ax, (int64_t)sizeof(double) * 3 * bv.atom_stride * R },
            { rec, rec ? (int64_t)sizeof(double) * MMC_RSTRIDE * n_mol * R : 0 },
            { bv.comq, bv.comq ? (int64_t)sizeof(uint16_t) * 3 * bv.cq_stride * R : 0 },
            { bv.S, (int64_t)sizeof(double) * 2 * nsb * MMC_NK_STRIDE * R },
            { bv.kxyz, (int64_t)sizeof(int32_t) * 3 * MMC_NK_STRIDE },
            { bv.cfac, (int64_t)sizeof(double) * MMC_NK_STRIDE },
            { bv.kmap, (int64_t)sizeof(int16_t) * 6 * 11 * 11 },
            { qq_tab, (int64_t)sizeof(double) * MMC_QQ_TABLE_DOUBLES },
            { kpack, (int64_t)sizeof(int32_t) * (MMC_NK_STRIDE + MMC_KCOLS) },
        };
        int64_t total = 0;
        for (const Seg &g : segs)
            total += (g.bytes + 15) / 16 * 16;
        MMC_TRY(dmalloc((void **)&snap.buf, (size_t)total));
        int64_t off = 0;
        int c = 0;
        for (const Seg &g : segs) {
            if (g.bytes == 0)
                continue;
            uint32_t *d = snap.buf + off / 4;
            snap.to_snap.dst[c] = d;
            snap.to_snap.src[c] = reinterpret_cast<const uint32_t *>(g.p);
            snap.to_snap.n[c] = g.bytes / 4;
            snap.from_snap.dst[c] = const_cast<uint32_t *>(reinterpret_cast<const uint32_t *>(g.p));
            snap.from_snap.src[c] = d;
            snap.from_snap.n[c] = g.bytes / 4;
            off += (g.bytes + 15) / 16 * 16;
            c++;
        }
        snap.to_snap.count = snap.from_snap.count = c;
    }
    k_copy_segments<<<512, 256, 0, stream>>>(snap.to_snap);
    MMC_HIP(hipGetLastError());
    snap.box = box; snap.kappa = bv.kappa; snap.nkvecs = nkvecs; snap.recip_order = recip_order;
    snap.valid = true;
    return MMC_OK;
}

int32_t DeviceSystem::snapshot_restore()
{
    MMC_REQUIRE(snap.valid, MMC_ERR_STATE, "no snapshot to restore");
    MMC_HIP(hipSetDevice(device));
    k_copy_segments<<<512, 256, 0, stream>>>(snap.from_snap);
    comq_epoch++;
    MMC_HIP(hipGetLastError());
    box = bv.box = snap.box;
    bv.kappa = snap.kappa;
    nkvecs = snap.nkvecs;
    bv.nkvecs = (int32_t)snap.nkvecs;
    recip_order = snap.recip_order;
    snap.valid = false;
    return MMC_OK;
}

// ---- per-replica boxes (mmc_perbox.inc) ----------------------------------------------------------
int32_t DeviceSystem::pb_upload_scalars()
{
    MMC_HIP(hipMemcpyAsync(pb.d_box, pb.box.data(), sizeof(double) * R, hipMemcpyHostToDevice, stream));
    MMC_HIP(hipMemcpyAsync(pb.d_kappa, pb.kappa.data(), sizeof(double) * R, hipMemcpyHostToDevice, stream));
    return sync(); // (pageable host arrays)
}

// cfac rows (PrepareEwaldVariables, ewalds.jl:45-103, over the shared k list) and erfc tables of
// the replicas in d_mask (NULL: all) for their current box and kappa
int32_t DeviceSystem::pb_build_tables(const int32_t *d_mask)
{
    dim3 gc((unsigned)((nkvecs + 63) / 64), (unsigned)R);
    k_cfac_pb<<<gc, 64, 0, stream>>>(bv.kxyz, (int)nkvecs, pb.d_kappa, pb.d_box, pb.cfac, d_mask,
                                     half_k ? 1 : 0);
    dim3 gt((unsigned)((MMC_QQ_NROW + 63) / 64), (unsigned)R);
    k_build_qq_table<<<gt, 64, 0, stream>>>(0.0, pb.tab, PerBoxTable{ pb.d_kappa, d_mask });
    MMC_HIP(hipGetLastError());
    return MMC_OK;
}

// take: copy the replicas in d_mask aside; else: copy them back.  Everything a volume trial
// rewrites: coordinates in their three layouts, the fixed-point centres of mass, both S(k)
// buffers, the cfac row and the table (box and kappa are the caller's, on the host).
int32_t DeviceSystem::pb_snapshot(const int32_t *d_mask, bool take)
{
    if (!pb.snap) {
        struct Seg { void *p; int64_t per; };
        const int nsb = R == 1 ? 4 : 2;
        const Seg segs[] = {
            { bv.comx, (int64_t)sizeof(double) * bv.mol_stride },
            { bv.comy, (int64_t)sizeof(double) * bv.mol_stride },
            { bv.comz, (int64_t)sizeof(double) * bv.mol_stride },
            { bv.ax, (int64_t)sizeof(double) * bv.atom_stride },
            { bv.ay, (int64_t)sizeof(double) * bv.atom_stride },
            { bv.az, (int64_t)sizeof(double) * bv.atom_stride },
            { rec, (int64_t)sizeof(double) * MMC_RSTRIDE * n_mol },
            { bv.comq, (int64_t)sizeof(uint16_t) * 3 * bv.cq_stride },
            { bv.S, (int64_t)sizeof(double) * 2 * nsb * MMC_NK_STRIDE },
            { pb.cfac, (int64_t)sizeof(double) * MMC_NK_STRIDE },
            { pb.tab, (int64_t)sizeof(double) * MMC_QQ_TABLE_DOUBLES },
        };
        int64_t total = 0;
        for (const Seg &g : segs)
            total += (g.per + 15) / 16 * 16 * R;
        MMC_TRY(dmalloc((void **)&pb.snap, (size_t)total));
        int64_t off = 0;
        int c = 0;
        for (const Seg &g : segs) {
            const int64_t per = (g.per + 15) / 16 * 16; // (every per-replica size is a multiple of 4 bytes)
            uint32_t *d = pb.snap + off / 4;
            pb.to_snap.dst[c] = d;
            pb.to_snap.src[c] = reinterpret_cast<const uint32_t *>(g.p);
            pb.to_snap.dst_stride[c] = per / 4;
            pb.to_snap.src_stride[c] = g.per / 4;
            pb.from_snap.dst[c] = reinterpret_cast<uint32_t *>(g.p);
            pb.from_snap.src[c] = d;
            pb.from_snap.dst_stride[c] = g.per / 4;
            pb.from_snap.src_stride[c] = per / 4;
            pb.to_snap.n[c] = pb.from_snap.n[c] = g.per / 4;
            off += per * R;
            c++;
        }
        pb.to_snap.count = pb.from_snap.count = c;
    }
    dim3 grid(64, (unsigned)R);
    k_copy_replicas<<<grid, 256, 0, stream>>>(take ? pb.to_snap : pb.from_snap, d_mask);
    if (!take)
        comq_epoch++;
    MMC_HIP(hipGetLastError());
    return MMC_OK;
}

// potential(..., "ewald") for every replica (energy.jl:946-1032)
int32_t DeviceSystem::totals_ewald(double lj_rcut, double qq_rcut, mmc_totals *tot, const TotalsHook *hook)
{
    MMC_REQUIRE(uploaded && ewald_ready, MMC_ERR_STATE,
                "potential needs an uploaded system and PrepareEwaldVariables");
    MMC_HIP(hipSetDevice(device));
    // everything is enqueued first and waited for once: pair kernels, structure factor, copies
    double sq, sq2;
    MMC_TRY(charge_sums(&sq, &sq2)); // cached after the first call
    std::vector<TotalsRaw> ht;
    std::vector<double> erec(R);
    bool fast = false;
    if (R == 1 && nk == 5 && !pb.on && !getenv("MMC_NO_POT_ONE")) { // one system: one launch (mmc_potential.hpp)
        fast = fast_table_ok(qq_rcut);
        PotOneOut o;
        MMC_TRY(potential_one(lj_rcut, qq_rcut, fast, true, &o));
        ht.resize(1);
        ht[0].lj_e = o.lj_e; ht[0].lj_v = o.lj_v; ht[0].qq = o.qq; ht[0].n_ovl = o.n_ovl; ht[0]._pad = 0;
        erec[0] = o.recip_e;
    } else {
        MMC_TRY(pair_totals_enqueue(lj_rcut, qq_rcut, ht, &fast));
        MMC_TRY(recip_long_enqueue(erec.data()));
        MMC_TRY(sync());
    }
    MMC_TRY(pair_totals_finish(lj_rcut, qq_rcut, ht, fast));
    if (hook)
        MMC_TRY(hook->fn(hook->ctx, ht, erec, &sq2));
    const double factor = bv.factor;
    for (int64_t r = 0; r < R; r++) {
        const double kappa = pb.on ? pb.kappa[r] : bv.kappa;
        const double self = -kappa * sq2 / sqrt(3.141592653589793) * factor; // ewalds.jl:832
        mmc_totals t;
        memset(&t, 0, sizeof(t));
        t.energy = ht[r].lj_e / 2; // energy.jl:978-980
        t.virial = ht[r].lj_v / 2;
        t.lj = ht[r].lj_e / 2;
        double totReal = ht[r].qq;
        totReal *= factor / 2;      // :1001
        t.energy += totReal; t.coulomb += totReal; t.virial += totReal / 3.0;
        t.real = totReal;
        double rec = erec[r] * factor; // :1009
        t.energy += rec; t.coulomb += rec; t.virial += rec / 3.0;
        t.recip = rec;
        t.energy += self; t.coulomb += self; t.virial += self / 3.0; // :1017-1021
        t.self = self;
        t.n_overlap = ht[r].n_ovl;
        if (pb.on && ht[r].n_ovl) { // (per-replica boxes: no per-molecule fallback, see mmc_hip.h)
            t.energy = INFINITY;
            t.n_overlap = 1;        // (a flag: the pair kernels do not count molecules)
        }
        tot[r] = t;
    }
    return MMC_OK;
}

// Copy one result record out of pinned host memory and accept it only if the copy carries the
// expected launch stamp and its checksum matches (store_part, mmc_kernels.hpp).
bool part_copy_checked(const PartOut *src, unsigned want_stamp, PartOut *dst)
{
    const volatile uint64_t *s = reinterpret_cast<const volatile uint64_t *>(src);
    uint64_t w[8];
    for (int k = 0; k < 8; k++)
        w[k] = s[k];
    memcpy(dst, w, sizeof(PartOut));
    if (part_stamp_of(dst->ovl[1]) != (want_stamp & MMC_STAMP_MASK))
        return false;
    return ((uint32_t)dst->ovl[0] >> 1) == part_checksum(reinterpret_cast<const double *>(dst), want_stamp);
}

extern "C" int32_t mmc_part_validate(const void *part_out_64, uint32_t stamp)
{
    if (!part_out_64)
        return 0;
    PartOut tmp;
    return part_copy_checked(reinterpret_cast<const PartOut *>(part_out_64), stamp, &tmp) ? 1 : 0;
}

void mmc_combine_parts(const PartOut *parts, int n_parts, double factor, mmc_move_result *res)
{
    double ljp[2] = { 0, 0 }, ljv[2] = { 0, 0 }, qq[2] = { 0, 0 }, rec = 0.0;
    int ov[2] = { 0, 0 };
    for (int p = 0; p < n_parts; p++) {
        for (int s = 0; s < 2; s++) {
            ljp[s] += parts[p].lj_pot[s];
            ljv[s] += parts[p].lj_vir[s];
            qq[s] += parts[p].qq_pot[s];
            ov[s] |= parts[p].ovl[s] & 1; // (ovl[1] carries the launch stamp above bit 0)
        }
        rec += parts[p].recip;
    }
    double e[2], v[2], qe[2], qv[2];
    for (int s = 0; s < 2; s++) {
        e[s] = ljp[s] * 4;          // energy.jl:289
        v[s] = ljv[s] * 24 / 3.0;
        double realEwald = ov[s] ? 0.0 : qq[s]; // ewalds.jl:359-360
        realEwald *= factor;                    // ewalds.jl:905
        qe[s] = realEwald;
        qv[s] = realEwald / 3;                  // ewalds.jl:907
    }
    const int overlap = ov[0] || ov[1];               // main.jl:574-578
    const double dRecip = overlap ? 0.0 : rec * factor; // main.jl:580-590, ewalds.jl:825
    res->d_lj = e[1] - e[0];
    res->d_real = qe[1] - qe[0];
    res->d_recip = dRecip;
    res->d_vir = ((v[1] + qv[1]) - (v[0] + qv[0])) + dRecip / 3; // main.jl:600-601
    res->overlap = overlap;
    res->_pad = 0;
}
