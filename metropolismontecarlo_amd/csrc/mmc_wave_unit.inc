// mmc_wave_unit.inc -- the body of one (replica, part) unit of the wave-per-move scheme: the
// reciprocal part, the COM scan, the pair loops and the 64-byte result record.  Included textually
// inside the unit loop of k_move_eval_wave (one unit per launch and wave) and inside the step loop
// of k_move_server_wave (one unit per wave for a whole run); see mmc_wave.hpp for the design.
//
// The including scope provides (all wave-uniform unless noted):
//   sm (WaveShared), wv, lane (per lane), bv, fc, pp, bc, same_gate, inv_box, gate_q, kpack, nkv, n_mol,
//   box, list, pvw, stamp;
//   w (per lane: word `lane` of the move record), i0 (chosen molecule, 0-based), scur (which S
//   buffer is sumQExpOld), pend (molecule whose accepted move is not in memory yet, or -1; its
//   record is in pvw), r (replica: selects the S buffers), myrec (the replica's records),
//   do_pairs, do_recip, j_begin, j_end; and as MACROS, expanded at their one point of use so that
//   they are not live across the unit: WV_CQ_BASE (the replica's fixed-point centres of mass) and
//   WV_PART_DST (where the PartOut goes; not needed with WV_UNIT_NO_STORE).
// WV_NS (default 2): states evaluated by the pair part.  2 = old and new (a trial move); 1 = only the
// "new" slot of the record (one LJ_poly_dU + EwaldReal of the molecule as the record gives it: the
// per-call surface of the context server): the old-state sums are left 0.
// With WV_UNIT_NO_STORE defined the record is not stored: sm.outw[wv][0..6] hold the seven sums and
// [7] the overlap bits (bit 0 old, bit 1 new) as an integer, for the includer to combine.
        // The seven sums of the unit are reduced and parked in LDS (outw) by the phase that
        // produces them, so no accumulator is live across phases.
#ifndef WV_NS
#define WV_NS 2
#define WV_NS_DEFAULTED
#endif
#if WV_NS == 2
#define WV_IF2(...) __VA_ARGS__
#else
#define WV_IF2(...)
#endif
#ifndef WV_SUBST // substitute the pending commit's words for its molecule (see k_move_eval_wave)
#define WV_SUBST 1
#define WV_SUBST_DEFAULTED
#endif
// WV_IMG (default 0): 1 = the minimum image of an atom pair taken with the image of its molecule's
// centre of mass (one subtraction and one fma per component instead of sub, sub, min).  Bit for bit
// the reference's vector1D for every pair inside a gate, PROVIDED gate + 2 r_mol < box / 2, r_mol =
// the largest distance of an atom from its molecule's centre of mass: a component of the COM vector
// of a gated pair is then either below gate (no wrap: every atom pair differs from it by less than
// 2 r_mol and does not wrap either) or above box - gate (wrap: every atom pair wraps the same way).
// The includer checks that on the host (mmc_batch.inc); lanes outside both gates compute garbage
// that every sum masks, as before.  The host also checks (gate + 2 r_mol)^2 < r_cut^2 + 100: every
// atom pair of a gated molecule pair then passes the slack tests of ewalds.jl:362 and energy.jl:270,
// and the one-state-per-pass pair loop does not make them.
#ifndef WV_IMG
#define WV_IMG 0
#define WV_IMG_DEFAULTED
#endif
#ifndef WV_PASSES // 1: both states of an atom pair together; 2: one state per pass over the records
#define WV_PASSES 1
#define WV_PASSES_DEFAULTED
#endif
#ifndef WV_ONE_CALL // 1: the pair loops have one call site, the scan is restarted per list (see the COM scan)
#define WV_ONE_CALL 0
#define WV_ONE_CALL_DEFAULTED
#endif
// WV_CAND (defined by k_move_eval_wave alone, a constant expression: true in its SUBST = false instantiations;
// not defined = 0): a step may fill the list from the chosen molecule's candidate list instead of scanning
// every centre of mass (see the COM scan).  Every other includer compiles exactly as without it.
#ifndef WV_XY // 1: the (kx, ky) products of the moved atoms once per column of k-vectors (see the k loop)
#define WV_XY 0
#define WV_XY_DEFAULTED
#endif
#ifndef WV_KPF // iterations of the k loop whose loads are in flight ahead of the one being computed
#define WV_KPF 2
#endif
#ifndef WV_WOLF // 1 (k_move_eval_wave's WOLF instantiations): no reciprocal part at all -- do_recip is
#define WV_WOLF 0 // false and sm has no phase tables but the reduction's scratch (WaveSharedT<.., false>)
#define WV_WOLF_DEFAULTED
#endif
#ifndef WV_ZERO // (a zero the includer can keep from being hoisted into a long-lived register pair)
#define WV_ZERO 0.0
#define WV_ZERO_DEFAULTED
#endif
#ifndef WV_VIRIAL // 0 (k_move_eval_wave's MULTI instantiations, whose record has no slot for it): the LJ
#define WV_VIRIAL 1 // virial is not computed; outw[2..3] stay the zeros the pair part starts from
#define WV_VIRIAL_DEFAULTED
#endif
#ifndef WV_STORE_IF // a step whose record is not stored makes neither its checksum nor its word 7
#define WV_STORE_IF true
#define WV_STORE_IF_DEFAULTED
#endif
#if WV_NS != 2
static_assert(WV_VIRIAL, "the one-state body always delivers the virial");
#endif
        double *const outw = sm.outw[wv];
        unsigned long long ovm0 = 0, ovm1 = 0; // lanes that saw an overlap, old / new state

        // ================= reciprocal part (ewalds.jl:718-826) =================
        // (Tried in round 4 and dropped: the k loop between the COM scan and the pair loops, the scan
        // ending with one load per lane that touches its neighbour's record, so that the gathers find
        // their lines in the L2 -- 290 us per launch instead of 270: the touches double the number of
        // line requests of the gathers, and those requests, not the trip to HBM, are what the gathers
        // cost.  Holding the gathered records in registers across the k loop spills at 96 VGPRs.)
        constexpr bool wv_wolf = WV_WOLF;
        if constexpr (!wv_wolf) {
        if (do_recip) {
            // phase tables e^{i 2 pi k x / L}, k = -5..5, of the 3 moved atoms, old and new: 18 rows
            {
                const int t = lane < 18 ? lane : 0;
                const int st = t / 9, q = t - 9 * st; // q = 3 l + d
                const double x = wave_pick(w, (st ? MV_AT_NEW : MV_AT_OLD) + q);
                if (lane < 18)
                    phase_row_moderate(x, box, sm.ptab[wv][st][q / 3][q % 3]);
            }
            wave_sync();
            WV_STAMP(2); // phase tables built
#ifdef WV_AFTER_PHASE_TABLES
            WV_AFTER_PHASE_TABLES
#endif
        }
        auto recip_loop = [&]() {
            double a_rec = 0;
#ifdef WV_S_BASE // (the context server names its buffers; there are more than two)
            const double *So = WV_S_BASE;
            double *Sn = WV_S_DST;
#else
            const double *So = s_buf(bv, r, scur);
            double *Sn = s_buf(bv, r, scur ^ 1);
#endif
            // Software pipeline of the k loop, WV_KPF iterations deep: the loads of iteration it + WV_KPF are in
            // flight during iteration it (one iteration is ~2 k cycles of this wave's share of its
            // SIMD, a trip to HBM more: one iteration ahead, as in round 3, every iteration waited --
            // stamps: 7.9 k of the loop's 19.9 k cycles), and the first are requested before the
            // column products are made.  No load or store of the loop sits in a branch (see the COM scan
            // below for why): lanes past the last k-vector redo vector nkv - 1 -- same value to
            // the same address -- and add it to the energy with weight zero.
            int kcs[WV_KPF], kps[WV_KPF];
            double cfs[WV_KPF];
            double2 sos[WV_KPF];
#pragma unroll
            for (int q = 0; q < WV_KPF; q++) {
                kcs[q] = min(lane + 64 * q, nkv - 1);
                kps[q] = kpack[kcs[q]];
                cfs[q] = bv.cfac[kcs[q]];
                sos[q] = *reinterpret_cast<const double2 *>(So + 2 * kcs[q]);
            }
#if WV_XY
            const int colp = kpack[MMC_NK_STRIDE + lane]; // the (kx, ky) of column `lane` (k_pack_kvec)
#endif
#if WV_XY
            // e^{i kx x} e^{i ky y} of the six (state, atom) once per COLUMN of k-vectors (lane c holds
            // column c; nk = 5, k^2 < 27 has 50 of them) instead of once per k-vector: the k loop fetches
            // its column's products from that lane (ds_bpermute) and multiplies by e^{i kz z} only --
            // the same two products in the same order, hence the same bits, for 24 instructions less
            // per 64 k-vectors.
            cplx xyp[2][3];
            {
                const int cx = colp & 15, cy = (colp >> 4) & 15;
#pragma unroll
                for (int st = 0; st < 2; st++)
#pragma unroll
                    for (int l = 0; l < 3; l++)
                        xyp[st][l] = c_mul_fused(sm.ptab[wv][st][l][0][5 + cx], sm.ptab[wv][st][l][1][cy]);
            }
#endif
#ifdef WV_S_MIRROR
            unsigned long long s_sum = 0; // integrity sum of the S_new words this wave sends to the host
#endif
            const int n_it = (nkv + 63) >> 6;
            int k = lane;
            for (int it = 0; it < n_it; it++) {
                const int kc = kcs[0], kp = kps[0];
                const double cf = cfs[0];
                const double2 so = sos[0];
#pragma unroll
                for (int q = 0; q + 1 < WV_KPF; q++) {
                    kcs[q] = kcs[q + 1]; kps[q] = kps[q + 1]; cfs[q] = cfs[q + 1]; sos[q] = sos[q + 1];
                }
                kcs[WV_KPF - 1] = min(k + 64 * WV_KPF, nkv - 1);
                kps[WV_KPF - 1] = kpack[kcs[WV_KPF - 1]];
                cfs[WV_KPF - 1] = bv.cfac[kcs[WV_KPF - 1]];
                sos[WV_KPF - 1] = *reinterpret_cast<const double2 *>(So + 2 * kcs[WV_KPF - 1]);
                {
                    const int kz = (kp >> 8) & 15;
                    double nr = so.x, ni = so.y;
#if WV_XY
                    const int col = (kp >> 12) & (MMC_KCOLS - 1);
                    auto from_col = [&](const cplx &v) {
                        cplx o;
                        o.re = wave_pick(v.re, col);
                        o.im = wave_pick(v.im, col);
                        return o;
                    };
#else
                    const int kx = kp & 15, ky = (kp >> 4) & 15;
#endif
#pragma unroll
                    for (int l = 0; l < 3; l++) {
#if WV_XY
                        const cplx tn = c_mul_fused(from_col(xyp[1][l]), sm.ptab[wv][1][l][2][kz]);
                        const cplx to = c_mul_fused(from_col(xyp[0][l]), sm.ptab[wv][0][l][2][kz]);
#else
                        const cplx tn = c_mul_fused(c_mul_fused(sm.ptab[wv][1][l][0][5 + kx], sm.ptab[wv][1][l][1][ky]),
                                                sm.ptab[wv][1][l][2][kz]);
                        const cplx to = c_mul_fused(c_mul_fused(sm.ptab[wv][0][l][0][5 + kx], sm.ptab[wv][0][l][1][ky]),
                                                sm.ptab[wv][0][l][2][kz]);
#endif
                        // (fused products and sums in this loop: see c_mul_fused)
                        nr = fma(fc.q[l], tn.re - to.re, nr); // ewalds.jl:805-814
                        ni = fma(fc.q[l], tn.im - to.im, ni);
                    }
                    *reinterpret_cast<double2 *>(Sn + 2 * kc) = make_double2(nr, ni);
#ifdef WV_S_MIRROR
                    { // sumQExpNew for the caller's array: write-through into the pinned mirror
                        typedef double s_piece __attribute__((ext_vector_type(2)));
                        s_piece v;
                        v.x = nr; v.y = ni;
                        double *mp = WV_S_MIRROR + 2 * kc;
                        asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" ::"v"(mp), "v"(v) : "memory");
                        if (k < nkv)
                            s_sum += (unsigned long long)__double_as_longlong(nr)
                                     + 3ULL * (unsigned long long)__double_as_longlong(ni);
                    }
#endif
                    const double wgt = k < nkv ? cf : 0.0;
                    a_rec = fma(wgt, fma(nr, nr, ni * ni) - fma(so.x, so.x, so.y * so.y), a_rec); // :817-821
                }
                k += 64;
            }
            wave_sum1_store(a_rec, &outw[6], outw, lane); // (scratch: outw[0..3], zeroed below before they count)
#ifdef WV_S_MIRROR
            s_sum = wave_sum_u64(s_sum);
            if (lane == 0) // (a reciprocal-only part: the pair sums of its record are unused)
                sm.pvw[wv][0] = __longlong_as_double((long long)s_sum);
#endif
            WV_STAMP(3); // reciprocal loop done
            wave_sync(); // ptab is rewritten by this wave's next unit
        };
        if (do_recip)
            recip_loop();
        } // !wv_wolf
        if (!do_recip && lane == 0)
            outw[6] = WV_ZERO;

        // ================= pair part =================
        if (do_pairs) {
            // The six sums live in registers only inside process(): each call reduces its own over
            // the wave and adds them to outw[0..5] (one call per unit unless the list overflows),
            // so nothing but the prefetch registers is live across the COM scan.
            if (lane < 6)
                outw[lane] = WV_ZERO;
            // The chosen molecule stays in the register `w` (lane t = word t of the move record);
            // its coordinates are pulled into SGPRs with v_readlane where they are used, so only
            // the six doubles of the current atom a (both states) are live in the pair loop.
            double cc[2][3]; // centres of mass, st 0 = old, 1 = proposal
            uint32_t cqxy[2], cqz[2]; // ... and their 16-bit box-fraction codes (com_quant), x | y << 16
            {
                const bool is_com = WV_IF2((lane >= MV_COM_OLD && lane < MV_COM_OLD + 3) ||)
                                    (lane >= MV_COM_NEW && lane < MV_COM_NEW + 3);
                const int myq = is_com ? (int)com_quant(w, inv_box) : 0;
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    WV_IF2(cc[0][d] = lane_f64(w, MV_COM_OLD + d);)
                    cc[1][d] = lane_f64(w, MV_COM_NEW + d);
                }
                WV_IF2(cqxy[0] = (uint32_t)lane_i32(myq, MV_COM_OLD) | (uint32_t)lane_i32(myq, MV_COM_OLD + 1) << 16;)
                cqxy[1] = (uint32_t)lane_i32(myq, MV_COM_NEW) | (uint32_t)lane_i32(myq, MV_COM_NEW + 1) << 16;
                WV_IF2(cqz[0] = (uint32_t)lane_i32(myq, MV_COM_OLD + 2);)
                cqz[1] = (uint32_t)lane_i32(myq, MV_COM_NEW + 2);
            }

            // ---- neighbours list[0 .. cnt): lane n takes neighbour n0 + n ----
            auto process = [&](int cnt) {
                WV_IF2(double a_lj0 = 0, a_v0 = 0, a_q0 = 0;)
                double a_lj1 = 0, a_v1 = 0, a_q1 = 0;
                wave_sync();
                for (int n0 = 0; n0 < cnt; n0 += 64) {
                    const int n = n0 + lane;
                    const int j = n < cnt ? list[n] : 0; // idle lanes: molecule 0, gates forced off
                    const bool act = (n < cnt) && (j != i0); // (the scan lets the chosen molecule through)
                    double t[MMC_REC];
                    const double2 *src = reinterpret_cast<const double2 *>(myrec + (int64_t)j * MMC_RSTRIDE);
#pragma unroll
                    for (int q = 0; q < 6; q++) {
                        const double2 v = src[q];
                        t[2 * q] = v.x;
                        t[2 * q + 1] = v.y;
                    }
                    if (n0 == 0)
                        WV_STAMP(5); // first neighbour records arrived
                    if (WV_SUBST && j == pend) {
#pragma unroll
                        for (int q = 0; q < MMC_REC; q++)
                            t[q] = pvw[q];
                    }
                    // the gates, exactly: COM minimum image of both states on the reference's
                    // arithmetic (energy.jl:248-254, ewalds.jl:334-340)
                    WV_IF2(bool g0, l0;)
                    bool g1, l1;
                    // (WV_IMG) m[st][d]: 0, or the sign of the COM difference where it exceeds half
                    // the box (vector1D's own choice, mmc_device.hpp): the image every atom pair
                    // of this neighbour takes in state st
                    constexpr bool wv_img = WV_IMG;
                    constexpr bool wv_virial = WV_VIRIAL;
                    double m[2][3] = { { 0, 0, 0 }, { 0, 0, 0 } };
                    auto min1 = [&](int st, int d, double a, double b) {
                        if constexpr (wv_img)
                            return fma(m[st][d], bc.neg, b - a); // == vector1D(a, b, bc), signed
                        else
                            return vector1D_abs(a, b, bc);
                    };
#define WV_MIN1(st, d, a, b) min1(st, d, a, b)
                    {
                        if constexpr (wv_img) {
#pragma unroll
                            for (int d = 0; d < 3; d++) {
                                const double d1 = t[9 + d] - cc[1][d];
                                m[1][d] = (fabs(d1) < bc.half) ? 0.0 : copysign(1.0, d1);
#if WV_NS == 2
                                const double d0 = t[9 + d] - cc[0][d];
                                m[0][d] = (fabs(d0) < bc.half) ? 0.0 : copysign(1.0, d0);
#endif
                            }
                        }
#if WV_NS == 2
                        const double x0 = WV_MIN1(0, 0, cc[0][0], t[9]), y0 = WV_MIN1(0, 1, cc[0][1], t[10]),
                                     z0 = WV_MIN1(0, 2, cc[0][2], t[11]);
                        const double c0 = x0 * x0 + y0 * y0 + z0 * z0;
                        g0 = act && (c0 < pp.qq_gate_sq); // ewalds.jl:340
                        l0 = same_gate ? g0 : (act && (c0 < pp.lj_gate_sq)); // energy.jl:254
#endif
                        const double x1 = WV_MIN1(1, 0, cc[1][0], t[9]), y1 = WV_MIN1(1, 1, cc[1][1], t[10]),
                                     z1 = WV_MIN1(1, 2, cc[1][2], t[11]);
                        const double c1 = x1 * x1 + y1 * y1 + z1 * z1;
                        g1 = act && (c1 < pp.qq_gate_sq);
                        l1 = same_gate ? g1 : (act && (c1 < pp.lj_gate_sq));
                    }
                    // the Coulomb gates as lane masks (one ballot per state and round): what is
                    // decided per atom pair below -- overlap, the cold path -- is then scalar
                    // mask arithmetic on the compare's own SGPR pair (a ballot of a COMBINED
                    // condition costs two VALU instructions per use: v_cndmask + v_cmp)
                    WV_IF2(const unsigned long long gm0 = wave_ballot(g0);)
                    const unsigned long long gm1 = wave_ballot(g1);
#if WV_PASSES == 2
// (no scheduling fence between the three b of an atom: with one state's temporaries the
// scheduler may start the next pair's table reads early and stays inside 96 VGPRs; -1.8 %)
#define WV_PAIR_FENCE
                    // ONE STATE PER PASS over the gathered records (old, then new): half the
                    // temporaries of the both-states form are live at a time, which is what lets the
                    // kernel be compiled for more waves per SIMD.  Same arithmetic, same order of
                    // the sums within a state.
                    //
                    // WHAT AN ATOM PAIR CLOSER THAN sqrt(ovr) CHANGES IS DECIDED ONCE PER ROUND AND STATE,
                    // not per atom pair.  The nine pairs are evaluated with the gate as their only mask
                    // and a running minimum of r^2 per lane; one test after them asks whether any gated
                    // lane came below ovr.  If none did -- every round of a healthy
                    // liquid -- the sums are bit for bit those of the exact body: the same fma chain in
                    // the same order, row 0 for the lanes outside the gate.  If one did, the Coulomb sum
                    // is put back to what it was when the round began and the round runs again through
                    // the exact body (overlap sentinel, series below the table), which leaves the LJ
                    // terms alone: those do not depend on it and have been added once already.
                    // Nothing is assumed about the system; only the speed depends on overlaps being rare.
                    auto pass = [&](auto stc, bool l, unsigned long long gm, unsigned long long &ovm,
                                    double &a_lj, double &a_v, double &a_q) {
                        constexpr int ST = decltype(stc)::value;
                        auto atoms = [&](auto exc, uint32_t &umin) {
                        constexpr bool EXACT = decltype(exc)::value;
#pragma unroll 1 // (unrolled: the per-pair constants are hoisted into VGPRs and spilled: 394 spills in round 4)
                        for (int a = 0; a < 3; a++) {
                            const int base_w = (ST ? MV_AT_NEW : MV_AT_OLD) + 3 * a;
                            const double ax = lane_f64(w, base_w), ay = lane_f64(w, base_w + 1),
                                         az = lane_f64(w, base_w + 2);
                            auto pair1 = [&](int ab, double bx, double by, double bz) {
                                const double qq = fc.qq9[ab];
                                const double px = WV_MIN1(ST, 0, ax, bx), py = WV_MIN1(ST, 1, ay, by),
                                             pz = WV_MIN1(ST, 2, az, bz);
                                const double u = px * px + py * py + pz * pz;
                                // (WV_IMG also promises (gate + 2 r_mol)^2 < r_cut^2 + 100: every atom pair of a gated
                                // molecule pair is inside the slack of ewalds.jl:362 / energy.jl:270, no need to look)
                                const unsigned long long km = (wv_img ? ~0ULL : wave_ballot(u < pp.qq_slack_sq)) & gm;
                                if constexpr (EXACT) {
                                    // opposite charges that close: the overlap sentinel (qm); like charges that
                                    // close: below r^2 = 0.25 the table ends (cold; practically never)
                                    const bool qneg = (fc.qneg_mask >> ab) & 1; // uniform
                                    const unsigned long long cm = wave_ballot(u < pp.ovr) & gm;
                                    const unsigned long long qm = qneg ? cm : 0ULL, cold = cm & ~qm;
                                    const unsigned long long im = km & ~qm;
                                    double e = qq_table_eval_lanes(sm.qtab, u, im);
                                    ovm |= qm;
                                    if (cold != 0ULL) {
                                        if (((im >> lane) & 1) && u < MMC_QQ_UMIN) e = qq_pair_cold(u, pp.kappa);
                                    }
                                    a_q = fma(e, qq, a_q); // ewalds.jl:365-367
                                } else {
                                umin = min(umin, (uint32_t)(__double_as_longlong(u) >> 32));
                                const double e = qq_table_eval_lanes(sm.qtab, u, km);
                                a_q = fma(e, qq, a_q); // ewalds.jl:365-367
                                // (the sum is pinned HERE: with no branch that needs e the compiler sinks the three
                                // Horner chains of an atom below the LJ branches, 60 registers of coefficients
                                // live at once, and spills the gathered records)
                                asm volatile("" : "+v"(a_q));
                                if ((fc.lj_mask >> ab) & 1) { // uniform (energy.jl:270: eps > 0.001); same r^2
                                    const double eps = fc.eps9[ab], sg = fc.sig9[ab];
                                    if (l && (wv_img || u < pp.lj_slack_sq)) {
                                        const double s2 = sg * sg / u;
                                        const double s6 = s2 * s2 * s2;
                                        const double s12 = s6 * s6;
                                        double f0, f1, f2; // (the pair's force, for the virial only)
                                        if constexpr (wv_virial) {
                                            const double virab = eps * (2.0 * s12 - s6);
                                            f0 = (wv_img ? px : vector1D(ax, bx, bc)) * virab * s2;
                                            f1 = (wv_img ? py : vector1D(ay, by, bc)) * virab * s2;
                                            f2 = (wv_img ? pz : vector1D(az, bz, bc)) * virab * s2;
                                        }
                                        a_lj += eps * (s12 - s6);
                                        if constexpr (wv_virial) {
                                            // COM vector of the virial (energy.jl:248-250, :279-281)
                                            a_v += (wv_img ? WV_MIN1(ST, 0, cc[ST][0], t[9]) : vector1D(cc[ST][0], t[9], bc)) * f0
                                                   + (wv_img ? WV_MIN1(ST, 1, cc[ST][1], t[10]) : vector1D(cc[ST][1], t[10], bc)) * f1
                                                   + (wv_img ? WV_MIN1(ST, 2, cc[ST][2], t[11]) : vector1D(cc[ST][2], t[11], bc)) * f2;
                                        }
                                    }
                                }
                                } // !EXACT
                            };
                            pair1(3 * a, t[0], t[1], t[2]);
                            WV_PAIR_FENCE
                            pair1(3 * a + 1, t[3], t[4], t[5]);
                            WV_PAIR_FENCE
                            pair1(3 * a + 2, t[6], t[7], t[8]);
                            WV_PAIR_FENCE
                        }
                        };
                        // The minimum is kept of the HIGH WORD of r^2 (r^2 >= +0: as an unsigned integer
                        // it orders as r^2 does; a NaN lies above every threshold, as in `u < ovr`) --
                        // one register and one 32-bit minimum per pair.  r^2 < ovr implies
                        // hi(r^2) <= hi(ovr): the test errs only towards the exact body.  The threshold
                        // is ovr itself: the exact body looks below the table's end (MMC_QQ_UMIN) only
                        // where r^2 < ovr (`cold` is a part of `cm`), so with no gated r^2 below ovr it
                        // does what the fast body did.  (max(ovr, MMC_QQ_UMIN) here is one more scalar
                        // register live across the pair loop: 151 spilled SGPRs, the parent has 150.)
                        const double a_q_in = a_q;
                        uint32_t umin = ~0u;
                        atoms(std::false_type{}, umin);
                        const uint32_t thr_hi = (uint32_t)(__double_as_longlong(pp.ovr) >> 32);
                        if (__builtin_expect((wave_ballot(umin <= thr_hi) & gm) != 0ULL, 0)) {
                            a_q = a_q_in;
                            atoms(std::true_type{}, umin);
                        }
                    };
                    WV_IF2(pass(std::integral_constant<int, 0>{}, l0, gm0, ovm0, a_lj0, a_v0, a_q0);)
                    pass(std::integral_constant<int, 1>{}, l1, gm1, ovm1, a_lj1, a_v1, a_q1);
                }
#else
                    // one atom pair (a, b), both states.  The Coulomb term needs only r^2, and
                    // (|d| - L)^2 == (d -+ L)^2 bit for bit, so the minimum image is taken on
                    // |d| (4 instructions per component instead of 6); the signed vector is
                    // rebuilt only inside the LJ branch, which few atom pairs enter.
                    auto pair_ab = [&](int ab, double a0x, double a0y, double a0z, double a1x,
                                       double a1y, double a1z, double bx, double by, double bz) {
                        const double qq = fc.qq9[ab];
                        const bool qneg = (fc.qneg_mask >> ab) & 1; // uniform
                        // which lanes are inside the gate and closer than sqrt(ovr) (cm), which
                        // count (im: ewalds.jl:359, :362): mask arithmetic on the compares' own
                        // SGPR pairs; the table returns 0 for the others (its row of zeros)
#if WV_NS == 2
                        const double p0x = WV_MIN1(0, 0, a0x, bx), p0y = WV_MIN1(0, 1, a0y, by),
                                     p0z = WV_MIN1(0, 2, a0z, bz);
                        const double u0 = p0x * p0x + p0y * p0y + p0z * p0z;
                        const unsigned long long cm0 = wave_ballot(u0 < pp.ovr) & gm0;
                        const unsigned long long im0 = wave_ballot(u0 < pp.qq_slack_sq) & (qneg ? gm0 & ~cm0 : gm0);
                        double e0 = qq_table_eval_lanes(sm.qtab, u0, im0);
#else
                        (void)a0x; (void)a0y; (void)a0z;
#endif
                        const double p1x = WV_MIN1(1, 0, a1x, bx), p1y = WV_MIN1(1, 1, a1y, by),
                                     p1z = WV_MIN1(1, 2, a1z, bz);
                        const double u1 = p1x * p1x + p1y * p1y + p1z * p1z;
                        const unsigned long long cm1 = wave_ballot(u1 < pp.ovr) & gm1;
                        const unsigned long long im1 = wave_ballot(u1 < pp.qq_slack_sq) & (qneg ? gm1 & ~cm1 : gm1);
                        double e1 = qq_table_eval_lanes(sm.qtab, u1, im1);
                        if (qneg) { // (uniform) opposite charges that close: the overlap sentinel
                            WV_IF2(ovm0 |= cm0;)
                            ovm1 |= cm1;
                        } else if ((WV_IF2(cm0 |) cm1) != 0ULL) {
                            // like charges closer than sqrt(ovr): below r^2 = 0.25 the table ends and
                            // the series takes over (practically never; UMIN <= ovr)
                            WV_IF2(if (((im0 >> lane) & 1) && u0 < MMC_QQ_UMIN) e0 = qq_pair_cold(u0, pp.kappa);)
                            if (((im1 >> lane) & 1) && u1 < MMC_QQ_UMIN) e1 = qq_pair_cold(u1, pp.kappa);
                        }
                        WV_IF2(a_q0 = fma(e0, qq, a_q0);) // ewalds.jl:365-367
                        a_q1 = fma(e1, qq, a_q1);
                        const double eps = fc.eps9[ab], sg = fc.sig9[ab];
                        if ((fc.lj_mask >> ab) & 1) { // uniform (energy.jl:270: eps > 0.001); same r^2
#if WV_NS == 2
                            if (l0 && u0 < pp.lj_slack_sq) {
                                const double s2 = sg * sg / u0;
                                const double s6 = s2 * s2 * s2;
                                const double s12 = s6 * s6;
                                double f0, f1, f2; // (the pair's force, for the virial only)
                                if constexpr (wv_virial) {
                                    const double virab = eps * (2.0 * s12 - s6);
                                    // (WV_IMG: the signed minimum image is what the distance was made of)
                                    f0 = (wv_img ? p0x : vector1D(a0x, bx, bc)) * virab * s2;
                                    f1 = (wv_img ? p0y : vector1D(a0y, by, bc)) * virab * s2;
                                    f2 = (wv_img ? p0z : vector1D(a0z, bz, bc)) * virab * s2;
                                }
                                a_lj0 += eps * (s12 - s6);
                                if constexpr (wv_virial) {
                                    // COM vector of the virial (energy.jl:248-250, :279-281)
                                    a_v0 += (wv_img ? WV_MIN1(0, 0, cc[0][0], t[9]) : vector1D(cc[0][0], t[9], bc)) * f0
                                            + (wv_img ? WV_MIN1(0, 1, cc[0][1], t[10]) : vector1D(cc[0][1], t[10], bc)) * f1
                                            + (wv_img ? WV_MIN1(0, 2, cc[0][2], t[11]) : vector1D(cc[0][2], t[11], bc)) * f2;
                                }
                            }
#endif
                            if (l1 && u1 < pp.lj_slack_sq) {
                                const double s2 = sg * sg / u1;
                                const double s6 = s2 * s2 * s2;
                                const double s12 = s6 * s6;
                                double f0, f1, f2; // (the pair's force, for the virial only)
                                if constexpr (wv_virial) {
                                    const double virab = eps * (2.0 * s12 - s6);
                                    f0 = (wv_img ? p1x : vector1D(a1x, bx, bc)) * virab * s2;
                                    f1 = (wv_img ? p1y : vector1D(a1y, by, bc)) * virab * s2;
                                    f2 = (wv_img ? p1z : vector1D(a1z, bz, bc)) * virab * s2;
                                }
                                a_lj1 += eps * (s12 - s6);
                                if constexpr (wv_virial) {
                                    a_v1 += (wv_img ? WV_MIN1(1, 0, cc[1][0], t[9]) : vector1D(cc[1][0], t[9], bc)) * f0
                                            + (wv_img ? WV_MIN1(1, 1, cc[1][1], t[10]) : vector1D(cc[1][1], t[10], bc)) * f1
                                            + (wv_img ? WV_MIN1(1, 2, cc[1][2], t[11]) : vector1D(cc[1][2], t[11], bc)) * f2;
                                }
                            }
                        }
                    };
#pragma unroll 1
                    for (int a = 0; a < 3; a++) {
#if WV_NS == 2
                        const double a0x = lane_f64(w, MV_AT_OLD + 3 * a),
                                     a0y = lane_f64(w, MV_AT_OLD + 3 * a + 1),
                                     a0z = lane_f64(w, MV_AT_OLD + 3 * a + 2);
#else
                        const double a0x = 0.0, a0y = 0.0, a0z = 0.0;
#endif
                        const double a1x = lane_f64(w, MV_AT_NEW + 3 * a),
                                     a1y = lane_f64(w, MV_AT_NEW + 3 * a + 1),
                                     a1z = lane_f64(w, MV_AT_NEW + 3 * a + 2);
                        // the three b are written out (static register indices) but scheduled one
                        // after the other: interleaving them costs 40 more VGPRs
                        pair_ab(3 * a, a0x, a0y, a0z, a1x, a1y, a1z, t[0], t[1], t[2]);
                        __builtin_amdgcn_sched_barrier(0);
                        pair_ab(3 * a + 1, a0x, a0y, a0z, a1x, a1y, a1z, t[3], t[4], t[5]);
                        __builtin_amdgcn_sched_barrier(0);
                        pair_ab(3 * a + 2, a0x, a0y, a0z, a1x, a1y, a1z, t[6], t[7], t[8]);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
#endif
#undef WV_MIN1
                // wave reduction (fixed order: bitwise reproducible)
#if WV_NS == 2
                if constexpr (WV_VIRIAL)
                    wave_sum6_add(a_lj0, a_lj1, a_v0, a_v1, a_q0, a_q1, outw, sm.sum6w(wv), lane);
                else
                    wave_sum4_add(a_lj0, a_lj1, a_q0, a_q1, outw, sm.sum6w(wv), lane);
#else
                const double s1 = wave_sum_rows(a_lj1), s3 = wave_sum_rows(a_v1), s5 = wave_sum_rows(a_q1);
                if (lane == 0) {
                    outw[1] += s1; outw[3] += s3; outw[5] += s5;
                }
#endif
                wave_sync();
            };

            // ---- COM scan, fixed-point prefilter of both states (com_quant: 16-bit box fractions,
            // whose wrapped difference IS the minimum image; the threshold gate_q admits every pair
            // the exact gate can accept): lane per molecule, survivors appended to the list in
            // ascending j.  WV_PF blocks of 64 molecules are in flight ahead of the one being tested
            // (static registers: the body is unrolled WV_PF times and block b's registers are
            // refilled as soon as it has been tested) ----
            // Addressing costs no vector instruction: the block pointers are scalars advanced once
            // per trip, every load is `scalar base + lane offset + immediate`.  Nothing is clamped:
            // the arrays end in MMC_CQ_PAD readable entries (mmc_system.inc), what lies beyond
            // j_end is masked where it is counted.
            const char *pxy = reinterpret_cast<const char *>(WV_CQ_BASE) + 4 * (int64_t)j_begin;
            const char *pz = reinterpret_cast<const char *>(WV_CQ_BASE + 2 * bv.cq_stride) + 2 * (int64_t)j_begin;
            const uint32_t ul4 = 4u * (uint32_t)lane, ul2 = 2u * (uint32_t)lane;
            // The unrolled body has no branch around a load: the s_waitcnt of a use can then name
            // exactly the loads it depends on, and WV_PF blocks really are in flight (with a load
            // or an early exit inside a branch the compiler must assume the fewest loads issued
            // since, and every test waited for the refill issued just before it).  The list is
            // checked for room once per WV_PF blocks, hence its size of 256 + 64 WV_PF.
            uint32_t pqxy = 0, pqz = 0; // codes of the pending commit's molecule (uniform)
            if (WV_SUBST && pend >= 0) {
                pqxy = (uint32_t)__builtin_amdgcn_readfirstlane((int)com_quant(pvw[9], inv_box))
                       | (uint32_t)__builtin_amdgcn_readfirstlane((int)com_quant(pvw[10], inv_box)) << 16;
                pqz = (uint32_t)__builtin_amdgcn_readfirstlane((int)com_quant(pvw[11], inv_box));
            }
            int base = j_begin, cnt = 0;
#ifdef WV_CAND
            // CANDIDATE LIST (mmc_cand.hpp; the includer provides cv, cand_on, d_cur, pcxy, pcz, n_cand; one part
            // per move: j_begin = 0, j_end = n_mol).  The chosen molecule's list names, in ascending j, every
            // molecule that can pass the prefilter while a + sqrt(D_r) stays inside the lists' budget: the SAME
            // test on the molecules' CURRENT codes is then made for those only -- at most MMC_CAND_CAP / 64
            // blocks instead of n_mol / 64 -- and list[0 .. cnt) is what the scan would have made.
            // Everything is requested at once, outside any branch (see below): the snapshot's codes of the
            // chosen molecule and of the one just committed, the list's length and its four blocks of
            // indices (scalar base + lane offset + immediate), then the codes gathered by index.  A step
            // that may not use them (bound run out, list overflowed, replica stale) has loaded 14 words
            // for nothing and scans.
#if WV_NS != 2 || !WV_ONE_CALL
#error "the candidate path: trial moves (WV_NS 2) and one call site of process() (WV_ONE_CALL)"
#endif
            bool cand_pre = false;
            if constexpr (WV_CAND) {
            if (cand_on) { // (uniform over the launch: the batch has lists)
                const int64_t cqs = bv.cq_stride;
                const uint16_t *ip = cv.idx + ((int64_t)r * n_mol + i0) * MMC_CAND_CAP;
                uint32_t cix[MMC_CAND_CAP / 64], gxy[MMC_CAND_CAP / 64], gz[MMC_CAND_CAP / 64];
#pragma unroll
                for (int b = 0; b < MMC_CAND_CAP / 64; b++)
                    cix[b] = ip[64 * b + lane];
                const int pm = pend >= 0 ? pend : i0; // (no branch around a load)
                const uint32_t qixy = cand_q0_xy(cv, cqs, r, i0), qiz = cand_q0_z(cv, cqs, r, i0);
                const uint32_t qpxy = cand_q0_xy(cv, cqs, r, pm), qpz = cand_q0_z(cv, cqs, r, pm);
                const uint32_t ccnt = cv.cnt[(int64_t)r * cqs + i0];
                const uint32_t *gpxy = reinterpret_cast<const uint32_t *>(WV_CQ_BASE);
                const uint16_t *gpz = WV_CQ_BASE + 2 * cqs;
#pragma unroll
                for (int b = 0; b < MMC_CAND_CAP / 64; b++) {
                    cix[b] = min(cix[b], (uint32_t)(n_mol - 1)); // (slots past the count: whatever they hold is readable)
                    gxy[b] = gpxy[cix[b]];
                    gz[b] = gpz[cix[b]];
                }
                // the commit this step wrote (its codes: pcxy, pcz) raises the replica's bound ...
                if (pend >= 0)
                    d_cur = (uint32_t)__builtin_amdgcn_readfirstlane(
                        (int)cand_note_commit(cv, qpxy, qpz, r, pcxy, pcz, d_cur, lane == 0));
                // ... and the one wave-uniform test, on the squares (cand_within)
                const uint32_t a2 = (uint32_t)__builtin_amdgcn_readfirstlane(
                    (int)max(com_quant_dist2(qixy, qiz, cqxy[0], cqz[0]), com_quant_dist2(qixy, qiz, cqxy[1], cqz[1])));
                const int ncand = __builtin_amdgcn_readfirstlane((int)ccnt);
                cand_pre = ncand <= MMC_CAND_CAP && cand_within(a2, d_cur, cv.budget);
                if (cand_pre) {
#pragma unroll
                    for (int b = 0; b < MMC_CAND_CAP / 64; b++) {
                        const bool keep = (64 * b + lane < ncand)
                                          && ((com_quant_dist2(gxy[b], gz[b], cqxy[0], cqz[0]) < gate_q)
                                              | (com_quant_dist2(gxy[b], gz[b], cqxy[1], cqz[1]) < gate_q));
                        const unsigned long long m = wave_ballot(keep);
                        if (keep)
                            list[cnt + lanes_below(m)] = (wv_list_t)cix[b];
                        cnt += __popcll(m);
                    }
                    base = j_end;
                    n_cand++;
                }
            }
            }
#endif
            uint32_t fxy[WV_PF], fz[WV_PF];
#if WV_ONE_CALL
            // ONE call site of process(): scan until the list has no room for another WV_PF blocks or
            // the range ends, take the list through the pair loops, and again while molecules remain
            // (the same neighbours in the same order and the same trips as with a call inside the scan
            // and one behind it, one copy of the pair loops instead of two).  The prefetch starts anew
            // with every list -- the blocks it re-reads were requested by the trip before -- so its
            // registers are not live across the pair loops.
#ifdef WV_CAND // (a list filled from the candidates goes through the same call of process(), once)
            while (cand_pre || base < j_end) {
            if (!cand_pre) {
            cnt = 0;
#else
            while (base < j_end) {
            cnt = 0;
#endif
#endif
#pragma unroll
            for (int b = 0; b < WV_PF; b++) {
                fxy[b] = *reinterpret_cast<const uint32_t *>(pxy + 256 * b + ul4);
                fz[b] = *reinterpret_cast<const uint16_t *>(pz + 128 * b + ul2);
            }
#if WV_ONE_CALL
            while (base < j_end && cnt <= WV_LIST - 64 * WV_PF) { // (no room for another WV_PF blocks: empty the list)
#else
            while (base < j_end) {
#endif
#pragma unroll
                for (int b = 0; b < WV_PF; b++) {
                    const int j = base + lane;
                    uint32_t xy = fxy[b], z = fz[b];
                    // refill this slot with the block WV_PF further on
                    fxy[b] = *reinterpret_cast<const uint32_t *>(pxy + 256 * (b + WV_PF) + ul4);
                    fz[b] = *reinterpret_cast<const uint16_t *>(pz + 128 * (b + WV_PF) + ul2);
                    if (WV_SUBST && j == pend) { xy = pqxy; z = pqz; }
                    const bool keep = WV_IF2((com_quant_dist2(xy, z, cqxy[0], cqz[0]) < gate_q) |)
                                      (com_quant_dist2(xy, z, cqxy[1], cqz[1]) < gate_q);
                    // Lanes past j_end are masked out of the COUNT only: they lie above every lane
                    // that counts, so what they append lands behind the block's last valid entry
                    // (room: the list is checked with 64 WV_PF slots to spare).  The chosen
                    // molecule itself passes (distance 0) and is dropped in process().
                    const int nv = j_end - base;
                    const unsigned long long m_end = nv >= 64 ? ~0ULL : (nv > 0 ? (1ULL << nv) - 1ULL : 0ULL);
                    const unsigned long long m = wave_ballot(keep);
                    if (keep)
                        list[cnt + lanes_below(m)] = j;
                    cnt += __popcll(m & m_end);
                    base += 64;
                }
                pxy += 256 * WV_PF;
                pz += 128 * WV_PF;
#if WV_ONE_CALL
            }
#ifdef WV_CAND
            }
            cand_pre = false;
#endif
            WV_STAMP(4); // scan done (the last list's, where there are several)
            if (cnt)
                process(cnt);
            }
#else
                if (cnt > WV_LIST - 64 * WV_PF) { // no room for another WV_PF blocks: empty the list
                    process(cnt);
                    cnt = 0;
                }
            }
            WV_STAMP(4); // scan done
            if (cnt)
                process(cnt);
#endif
            WV_STAMP(6); // pair loops done
        } else if (lane < 6) {
            outw[lane] = WV_ZERO;
        }
#ifdef WV_S_MIRROR
        if (do_recip && !do_pairs) {
            wave_sync();
            if (lane == 0)
                outw[0] = sm.pvw[wv][0]; // the integrity sum of the mirrored S_new (raw bits)
        }
#endif

#ifdef WV_UNIT_NO_STORE
        // the includer combines the parts itself: leave the sums and the raw overlap bits in outw
        if (lane == 0)
            outw[7] = __longlong_as_double((long long)((ovm0 != 0ULL ? 1 : 0) | (ovm1 != 0ULL ? 2 : 0)));
#else
        // ---- the 64-byte result record ----
        wave_sync();
        {   // seven lanes hash a word each (part_checksum_lanes)
#ifdef WV_DECIDE // the includer makes the accept decision here (k_move_eval_wave); it may replace
                 // the seven sums by what it wants sent instead (several steps per launch)
            const int accept = WV_DECIDE(ovm0 != 0ULL, ovm1 != 0ULL);
#else
            const int accept = 0;
#endif
            if (WV_STORE_IF) {
                const uint32_t csum = part_checksum_lanes(lane < 7 ? outw[lane] : 0.0, lane, stamp);
#ifdef WV_RECORD_OVL // (... and the overlap bits of the record it sends)
                if (lane == 0)
                    outw[7] = pack_ovl(WV_RECORD_OVL(ovm0 != 0ULL), WV_RECORD_OVL(ovm1 != 0ULL), stamp, csum, accept);
#else
                if (lane == 0)
                    outw[7] = pack_ovl(ovm0 != 0ULL, ovm1 != 0ULL, stamp, csum, accept);
#endif
            }
        }
        wave_sync();
#ifdef WV_STORE_WT // a persistent kernel: the host waits for this record while the kernel lives
        store_part<true>(WV_PART_DST, sm.outw[wv], lane);
#else
#ifndef WV_STORE_SYSTEM // (true: system-scope stores -- the host sees the record when the unit ends, not
#define WV_STORE_SYSTEM false // when the L2 writes it back, which may be as late as the end of the kernel)
#define WV_STORE_SYSTEM_DEFAULTED
#endif
        if (WV_STORE_IF)
            store_part<WV_STORE_SYSTEM>(WV_PART_DST, sm.outw[wv], lane);
#ifdef WV_STORE_SYSTEM_DEFAULTED
#undef WV_STORE_SYSTEM
#undef WV_STORE_SYSTEM_DEFAULTED
#endif
#endif
        wave_sync();
        WV_STAMP(7); // result stored
#endif
#ifdef WV_STORE_IF_DEFAULTED
#undef WV_STORE_IF
#undef WV_STORE_IF_DEFAULTED
#endif
#undef WV_IF2
#ifdef WV_XY_DEFAULTED
#undef WV_XY
#undef WV_XY_DEFAULTED
#endif
#ifdef WV_ONE_CALL_DEFAULTED
#undef WV_ONE_CALL
#undef WV_ONE_CALL_DEFAULTED
#endif
#ifdef WV_PASSES_DEFAULTED
#undef WV_PASSES
#undef WV_PASSES_DEFAULTED
#endif
#ifdef WV_IMG_DEFAULTED
#undef WV_IMG
#undef WV_IMG_DEFAULTED
#endif
#ifdef WV_SUBST_DEFAULTED
#undef WV_SUBST
#undef WV_SUBST_DEFAULTED
#endif
#ifdef WV_ZERO_DEFAULTED
#undef WV_ZERO
#undef WV_ZERO_DEFAULTED
#endif
#ifdef WV_VIRIAL_DEFAULTED
#undef WV_VIRIAL
#undef WV_VIRIAL_DEFAULTED
#endif
#ifdef WV_WOLF_DEFAULTED
#undef WV_WOLF
#undef WV_WOLF_DEFAULTED
#endif
#ifdef WV_NS_DEFAULTED
#undef WV_NS
#undef WV_NS_DEFAULTED
#endif
