// mmc_engine.inc -- the native host driver: Loop()'s sequential accept/reject (Ewald/main.jl:487-644)
// for every replica, in C++ on the host, around the batch's fused move kernel.
// Included by mmc_hip.hip after mmc_batch.inc.
//
// Shape: the replicas are cut into G groups (default 2 = double buffering), each with its own HIP
// stream.  For one group a step is: wait for its kernel -> Metropolis for its replicas -> next
// proposals -> H2D copy + launch.  While the host does that for group A, group B's kernel fills
// the GPU.  The per-replica host work of a group (Metropolis + proposal, ~80 ns per replica) is
// split over T threads with a spin barrier; thread 0 owns the HIP calls.  Nothing is shared
// between replicas, so slices need no locks.
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <mutex>
#include <thread>

#ifndef MMC_HOST_CHUNK
#define MMC_HOST_CHUNK 128 // replicas of a group's tail a host thread takes at a time (Driver::share)
#endif

namespace {

struct Rng { // xoshiro256++ seeded by splitmix64; one independent stream per replica
    uint64_t s[4];
    static uint64_t splitmix(uint64_t &x)
    {
        uint64_t z = (x += 0x9e3779b97f4a7c15ULL);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
        return z ^ (z >> 31);
    }
    void seed(uint64_t v)
    {
        for (int k = 0; k < 4; k++)
            s[k] = splitmix(v);
    }
    static inline uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
    inline uint64_t next()
    {
        const uint64_t result = rotl(s[0] + s[3], 23) + s[0];
        const uint64_t t = s[1] << 17;
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3];
        s[2] ^= t;
        s[3] = rotl(s[3], 45);
        return result;
    }
    inline double uniform() { return (double)(next() >> 11) * 0x1.0p-53; } // [0, 1)
};

// boundaries.jl:16-26
inline double pbc1(double x, double box)
{
    if (x > box) x -= box;
    if (x < 0) x += box;
    return x;
}

// One proposal for a molecule whose current state is com/at.
// Translation: random_translate_vector (auxillary.jl:94-103), the atoms follow the centre of mass
// rigidly.  Rotation: random axis by rejection (quaternions.jl:52-74), angle uniform in
// +-dphi_max (:176), applied to the atom offsets about the centre of mass.
// Returns 0 for a translation, 1 for a rotation.
inline int propose(Rng &g, double dr_max, double dphi_max, double box, const double *com,
                   const double *at, double *com_new, double *at_new)
{
    const double chose_move = g.uniform(); // main.jl:516
    if (chose_move < 0.5) {
        double d[3];
        for (int k = 0; k < 3; k++) {
            const double zeta = g.uniform() - 0.5;
            com_new[k] = pbc1(com[k] + zeta * dr_max, box);
            d[k] = com_new[k] - com[k];
        }
        for (int a = 0; a < 3; a++)
            for (int k = 0; k < 3; k++)
                at_new[3 * a + k] = at[3 * a + k] + d[k];
        return 0;
    }
    double e[3], norm;
    do {
        for (int k = 0; k < 3; k++)
            e[k] = 2.0 * g.uniform() - 1.0;
        norm = e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
    } while (!(norm < 1.0) || norm == 0.0);
    const double inv = 1.0 / std::sqrt(norm);
    for (int k = 0; k < 3; k++)
        e[k] *= inv;
    const double angle = (2.0 * g.uniform() - 1.0) * dphi_max;
    const double c = std::cos(angle), s = std::sin(angle), t = 1.0 - c;
    const double Rm[3][3] = {
        { t * e[0] * e[0] + c, t * e[0] * e[1] - s * e[2], t * e[0] * e[2] + s * e[1] },
        { t * e[0] * e[1] + s * e[2], t * e[1] * e[1] + c, t * e[1] * e[2] - s * e[0] },
        { t * e[0] * e[2] - s * e[1], t * e[1] * e[2] + s * e[0], t * e[2] * e[2] + c } };
    for (int k = 0; k < 3; k++)
        com_new[k] = com[k];
    for (int a = 0; a < 3; a++) {
        const double o[3] = { at[3 * a] - com[0], at[3 * a + 1] - com[1], at[3 * a + 2] - com[2] };
        for (int k = 0; k < 3; k++)
            at_new[3 * a + k] = com[k] + Rm[k][0] * o[0] + Rm[k][1] * o[1] + Rm[k][2] * o[2];
    }
    return 1;
}

struct SpinBarrier { // sense-reversing; the driver's threads are never oversubscribed on purpose
    std::atomic<int> count{ 0 };
    std::atomic<int> sense{ 0 };
    int n = 1;
    void wait(int &local)
    {
        local ^= 1;
        if (count.fetch_add(1, std::memory_order_acq_rel) == n - 1) {
            count.store(0, std::memory_order_relaxed);
            sense.store(local, std::memory_order_release);
        } else {
            int spins = 0;
            while (sense.load(std::memory_order_acquire) != local)
                if (++spins > 2000)
                    std::this_thread::yield();
        }
    }
};

// What a call will do, decided by run_plan from the batch's options and the call's parameters before
// anything is touched: the Driver only reads it.
struct RunPlan {
    int G = 0;                   // groups of replicas, each with its own launches
    struct { int64_t r0, nr; int kernel; } group[MMC_MAX_GROUPS]; // replicas [r0, r0 + nr) and their move kernel (batch_kernel_for)
    int n_streams = 1;           // group g launches on stream g % n_streams
    int T = 1;                   // host threads
    int P = 1;                   // result records per move the move kernel writes
    bool solute = false;         // a fixed solute (mmc_batch_set_solute): one more record per move, k_solute_move's
    int records() const { return P + (solute ? 1 : 0); } // ... and what the host reads and adds up
    bool devgen = false;         // proposals generated on the device (mmc_propose.hpp)
    bool server = false;         // the persistent move server does the launches' work
    int server_waves = 0;        // ... with this many parts (waves of a replica's workgroup)
    int server_lat_wgs = 0;      // > 0: the latency server, this many workgroups per replica
    bool devacc = false;         // the accept decision made by the move kernel itself (thread_main_devacc)
    int K = 1;                   // ... which then takes every replica through K steps per launch (DecideConsts)
    int gen_max = MMC_GEN_MAX;   // steps one k_propose launch draws (a whole call's: K, run_plan)
    bool cand = false;           // some group runs the wave kernel with one part per move: its candidate lists (mmc_cand.hpp)
    bool no_tail_share = true;   // Driver::share: every thread one contiguous slice
};

struct Group {
    int64_t r0 = 0, nr = 0;
    int kernel = 0;        // the move kernel of its launches (RunPlan)
    hipStream_t stream = nullptr;
    hipStream_t launched_on = nullptr; // the stream of its launch in flight (the first may ride on another group's: prelaunch)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int buf = 0;           // h_moves[buf] holds the proposals in flight (after the first launch)
    int64_t gen_end = 0;   // device proposals: records of steps < gen_end exist in the ring
    unsigned long long n_launch = 0; // launches enqueued in this run
    unsigned stamp = 0;    // stamp of the launch in flight (PartOut::ovl[1], see store_part)
    bool timed = false;    // the launch in flight is bracketed by ev0 / ev1
    std::chrono::steady_clock::time_point t_post; // move server: when the step's words were posted
};

// adjust.jl:1-41 (Adjust!) and :43-83 (Adjust_rot!, the same body)
inline void adjust_step(int64_t &naccepp, int64_t &attempp, int64_t naccept, int64_t attempt,
                        double set_value, double L, double &d_max)
{
    if (attempp == 0) { // :3-5: the first call only records
        naccepp = naccept;
        attempp = attempt;
        return;
    }
    if (attempt == attempp)
        return; // no attempt since the last call: the reference's ratio would be 0/0
    const double ratio = (double)(naccept - naccepp) / (double)(attempt - attempp);
    const double dr_old = d_max;
    d_max = d_max * ratio / set_value;
    const double dr_ratio = d_max / dr_old;
    if (dr_ratio > 1.5) d_max = dr_old * 1.5;
    if (dr_ratio < 0.5) d_max = dr_old * 0.5;
    if (d_max > L / 2) d_max = L / 2;
    naccepp = naccept;
    attempp = attempt;
}

struct Driver {
    const RunPlan plan;
    explicit Driver(const RunPlan &pl) : plan(pl) {}
    mmc_batch *b;
    const mmc_run_params *p;
    double *energies;          // mmc_batch_run
    const double *temps = nullptr; // per-replica temperatures (mmc_batch_set_temperatures), or null: p->temperature
    mmc_chain *chains = nullptr; // mmc_batch_run_chains
    int adjust = 0;
    uint8_t s_flip = 1;          // an accepted move hands the S buffers over (main.jl:621); 0 in Wolf style,
                                 // whose moves leave both where they were
    std::vector<Group> groups;
    std::vector<Rng> rng;
    std::vector<uint8_t> acc_prev, kind;
    PairParams pp;
    SpinBarrier bar;
    std::atomic<int32_t> status{ MMC_OK };
    std::atomic<int> drained_polls{ 0 };
    char err[256] = "";
    std::vector<mmc_run_stats> tstats; // one per thread
    std::vector<double> trace_t;       // MMC_RUN_TRACE: microseconds since the call began at each launch
    std::chrono::steady_clock::time_point trace_t0;
    std::vector<double> entry_t;       // MMC_RUN_TRACE: when each thread had entered thread_main
    std::vector<double> mark_t;        // MMC_RUN_TRACE: thread 0 after each pass of the first iterations
    double now_us() const { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - trace_t0).count(); }
    int64_t rng_off = 0;               // steps this batch had run before the call
    std::atomic<int> inject_left{ 0 }; // test hook "inject_torn"

    ChainKey chain_key(int64_t r) const
    {
        return ChainKey{ p->seed, (uint32_t)(p->replica0 + (uint64_t)r) };
    }

    // ---- per-replica host work ------------------------------------------------------------
    // One look at replica r's P result records: all of them carry `want` and pass their checksum
    // (copied to parts[]) or not yet.  A record is complete when it carries the launch's stamp AND
    // the checksum of the bytes copied out of it matches (store_part: the four 16-byte pieces of
    // the device's store may land separately; a torn record fails the checksum and is read again).
    // Returns 1 = collected, 0 = not yet, -1 = the run has failed (test hook, see below).
    // slot: the half of h_parts the launch wrote (1: the kernel's own decisions only, P == 1).
    int collect(int64_t r, unsigned want, PartOut *parts, int &q_done, mmc_run_stats &st, int slot = 0)
    {
        for (; q_done < plan.records(); q_done++) {
            const PartOut *src = q_done < plan.P ? &b->h_parts[(size_t)slot * b->sys.R + r * plan.P + q_done]
                                                 : &b->sol.h_parts[r]; // (the host decides: slot 0)
            if (part_stamp_of(*(const volatile int32_t *)&src->ovl[1]) != want)
                return 0;
            std::atomic_thread_fence(std::memory_order_acquire);
            if (inject_left.load(std::memory_order_relaxed) > 0 && inject_left.fetch_sub(1) > 0) {
                // what a torn write looks like: the stamp piece is new, another 16-byte piece
                // still holds the previous launch's bytes
                PartOut torn;
                memcpy(&torn, (const void *)src, sizeof(torn));
                torn.lj_vir[q_done & 1] += 1.0;
                if (!part_copy_checked(&torn, want, &parts[q_done])) {
                    st.torn_records++;
                    return 0;
                }
                mmc_set_error("a corrupted result record passed the checksum");
                fail(MMC_ERR_HIP);
                return -1;
            }
            if (!part_copy_checked(src, want, &parts[q_done])) {
                st.torn_records++;
                return 0;
            }
        }
        return 1;
    }

    // Where a thread keeps what it writes per replica and step: the batch's own arrays, or -- on
    // the move server, where several threads write every few microseconds -- copies of its slice
    // (the arrays are bytes and doubles: a cache line holds 64 or 8 replicas' worth, and threads
    // writing neighbours' lines made eight threads slower than two).  Element of replica r: [r - off].
    struct RepView {
        uint8_t *acc, *kind, *scur, *flags;
        double *energy;
        int64_t off;
    };
    RepView global_view()
    {
        return RepView{ acc_prev.data(), kind.data(), b->s_cur.data(), b->h_flags, energies, 0 };
    }

    // The decision on replica r's step `step_done` from its records (main.jl:593-651).
    void decide(int64_t r, const PartOut *parts, int64_t step_done, mmc_run_stats &st, int dev_accept = -1)
    {
        decide(r, parts, step_done, st, global_view(), dev_accept);
    }
    // dev_accept >= 0: the decision the kernel made (DecideConsts); the bookkeeping is the same
    void decide(int64_t r, const PartOut *parts, int64_t step_done, mmc_run_stats &st, const RepView &v,
                int dev_accept = -1)
    {
        const double T_ = temps ? temps[r] : p->temperature, factor = b->sys.bv.factor;
        const bool sweep_end = (step_done % b->sys.n_mol) == b->sys.n_mol - 1;
        mmc_move_result res;
        mmc_combine_parts(parts, plan.records(), factor, &res);
        const double delta = res.d_lj + res.d_real + res.d_recip; // main.jl:593
        if (res.overlap)
            st.overlaps++; // main.jl:595-597
        // Metropolis(delta / temperature) && overlap == false (main.jl:598, auxillary.jl:106-114)
        const double x = delta / T_;
        bool met;
        if (dev_accept >= 0) met = dev_accept != 0;
        else if (x < 0.0) met = true;
        else met = std::exp(-x) > (plan.devgen ? mmc_metropolis_uniform(chain_key(r), (uint64_t)(rng_off + step_done))
                                               : rng[r].uniform());
        const bool accept = met && !res.overlap;
        if (step_done < b->trace_steps) { // test hook "trace_steps"
            b->trace_delta[(size_t)r * b->trace_steps + step_done] = delta;
            b->trace_flags[(size_t)r * b->trace_steps + step_done] =
                (uint8_t)((accept ? 1 : 0) | (res.overlap ? 2 : 0) | (v.kind[r - v.off] ? 4 : 0));
        }
        const uint8_t kind_r = v.kind[r - v.off];
        if (kind_r == 0) st.trans_attempt++; else st.rot_attempt++;
        if (accept) {
            if (kind_r == 0) st.trans_accept++; else st.rot_accept++;
        }
        v.acc[r - v.off] = accept ? 1 : 0;
        st.moves++;
        if (!chains) {
            if (accept)
                v.energy[r - v.off] += delta; // main.jl:599
            return;
        }
        mmc_chain &c = chains[r];
        if (res.overlap) c.overlaps++;
        if (kind_r == 0) c.trans_attempt++; else c.rot_attempt++; // main.jl:521,530
        if (accept) {
            c.energy += delta;     // main.jl:599
            c.virial += res.d_vir; // main.jl:600-601
            if (kind_r == 0) c.trans_naccept++; else c.rot_naccept++;
        }
        c.avg_energy += c.energy; // main.jl:606-613 (accepted) / :624-625 (rejected)
        c.avg_virial += c.virial;
        c.steps_taken++;          // main.jl:641
        if (sweep_end && adjust) { // main.jl:645-651
            adjust_step(c.trans_naccepp, c.trans_attempp, c.trans_naccept, c.trans_attempt,
                        c.trans_set_value, b->sys.box, c.dr_max);
            adjust_step(c.rot_naccepp, c.rot_attempp, c.rot_naccept, c.rot_attempt,
                        c.rot_set_value, b->sys.box, c.dphi_max);
            if (plan.devgen)
                b->h_steps[r] = make_double2(c.dr_max, c.dphi_max);
        }
    }

    // [lo, hi) of a group, step `step_done`: waits for every replica's records in turn.
    // gated: wait on the LAST record first.  A line the host has read before the GPU writes it
    // costs that write a probe into a core's cache; a thread that keeps pace with the kernel does
    // that to every record it takes (all threads working through interleaved chunks of 128 from the
    // start: the launch ran 15 % longer, round 4).  Gated it happens to one line of the chunk, and
    // the rest -- written in the same round of the kernel -- is almost always there in its turn.
    // Device-side decisions: the records carry the decision; the host adds the step's bookkeeping (and
    // the kind of the move, for the counts).  slot: the half of h_parts the launch wrote (collect).
    void metropolis(const Group &g, int64_t lo, int64_t hi, int64_t step_done, mmc_run_stats &st,
                    bool gated = false, int slot = 0)
    {
        const unsigned want = g.stamp & MMC_STAMP_MASK;
        if (gated && hi > lo) {
            const PartOut *gate = &b->h_parts[(size_t)slot * b->sys.R + (hi - 1) * plan.P + (plan.P - 1)];
            for (unsigned spins = 1; part_stamp_of(*(const volatile int32_t *)&gate->ovl[1]) != want; spins++) {
                if (((spins & 0xffff) == 0 && !still_running(g)) || status.load(std::memory_order_relaxed) != MMC_OK)
                    return;
                for (int k = 0; k < 16; k++)
                    mmc_cpu_relax();
            }
        }
        for (int64_t r = lo; r < hi; r++) {
            PartOut parts[MMC_MAX_PARTS + 1];
            int q_done = 0;
            for (unsigned spins = 1;; spins++) {
                const int c = collect(r, want, parts, q_done, st, slot);
                if (c > 0)
                    break;
                if (c < 0 || ((spins & 0xfffff) == 0 && !still_running(g)))
                    return;
                mmc_cpu_relax(); // (a polling core that hammers the line the GPU is about to write slows that write)
            }
            const int64_t n_sub = plan.devacc ? std::min<int64_t>(plan.K, p->n_steps - step_done) : 1;
            if (n_sub > 1) { // one record for the launch's steps [step_done, step_done + n_sub)
                unsigned long long bits, kbits;
                memcpy(&bits, &parts[0].lj_pot[1], 8);
                memcpy(&kbits, &parts[0].lj_vir[0], 8);
                const unsigned acc_mask = (unsigned)bits, ovl_mask = (unsigned)(bits >> 32),
                               kind_mask = (unsigned)kbits; // (the record's words: DecideConsts)
                energies[r] += parts[0].lj_pot[0]; // the accepted steps' dU, added up in step order by the kernel
                for (int64_t k = 0; k < n_sub; k++) {
                    const int kd = (kind_mask >> k) & 1; // (what k_propose drew: mmc_move_kind of that step)
                    const bool acc = (acc_mask >> k) & 1;
                    if (kd == 0) { st.trans_attempt++; st.trans_accept += acc; }
                    else { st.rot_attempt++; st.rot_accept += acc; }
                    st.overlaps += (ovl_mask >> k) & 1;
                    if (acc && step_done + k + 1 < p->n_steps)
                        b->s_cur[r] ^= s_flip; // main.jl:621 (the call's last step: settle_slice)
                    if (k + 1 == n_sub) {
                        acc_prev[r] = acc ? 1 : 0;
                        kind[r] = (uint8_t)kd;
                    }
                }
                st.moves += n_sub;
            } else if (plan.devacc) {
                kind[r] = (uint8_t)mmc_move_kind(chain_key(r), (uint64_t)(rng_off + step_done));
                decide(r, parts, step_done, st, part_accept_of(parts[0].ovl[1]));
                if (acc_prev[r] && step_done + 1 < p->n_steps)
                    b->s_cur[r] ^= s_flip; // main.jl:621 (the last step's: settle_slice)
            } else
                decide(r, parts, step_done, st);
        }
    }

    // Thread t's share of a group.  Host-side decisions: ONE contiguous slice.  The persistent
    // kernel works through its units in index order, 5120 at a time, so the owner of the last slice
    // gets its records in the kernel's last round and works ~200 us beyond the kernel's end (4096
    // records at ~50 ns); the two-group pipeline hides that behind the other group's kernel, and
    // every other split tried in round 4 was no better: chunks of 64-512 dealt out in turn from the
    // start ran the LAUNCH 5-25 % longer (threads that keep pace with the kernel read lines the GPU
    // is about to write: see metropolis), and a contiguous 7/8 + a dealt-out last eighth measured
    // the same as this -- a thread's 200 us per launch is the cost, not its order.
    // Device-side decisions: the last eighth (tail_div) dealt out in chunks of MMC_HOST_CHUNK (the
    // bookkeeping is light, and nothing waits for it but the end of the call).
    // fn(lo, hi, gated): gated = a chunk of the tail (see metropolis).
    static constexpr int tail_div = 8;
    template <class F> void share(const Group &g, int t, F &&fn) const
    {
        const int64_t tail = g.nr >= 16 * (int64_t)MMC_HOST_CHUNK * plan.T && !plan.no_tail_share ? g.nr / tail_div : 0;
        const int64_t bulk = g.nr - tail;
        if (bulk * t / plan.T < bulk * (t + 1) / plan.T)
            fn(g.r0 + bulk * t / plan.T, g.r0 + bulk * (t + 1) / plan.T, false);
        const int64_t n_chunks = (tail + MMC_HOST_CHUNK - 1) / MMC_HOST_CHUNK;
        for (int64_t c = t; c < n_chunks; c += plan.T) {
            const int64_t lo = g.r0 + bulk + c * MMC_HOST_CHUNK;
            fn(lo, std::min(lo + (int64_t)MMC_HOST_CHUNK, g.r0 + g.nr), true);
        }
    }

    void proposals(const Group &g, int64_t lo, int64_t hi, int64_t step, int buf)
    {
        DeviceSystem &s = b->sys;
        MoveRec *cur = b->h_moves[buf];
        const MoveRec *prev = b->h_moves[buf ^ 1];
        const int mol = (int)(step % s.n_mol) + 1; // main.jl:490: `for i = 1:numbers.molecules`
        if (plan.devgen) { // the device draws the move; the host only says what became of the last one
            for (int64_t r = lo; r < hi; r++) {
                if (acc_prev[r])
                    b->s_cur[r] ^= s_flip; // main.jl:621
                b->h_flags[r] = (uint8_t)((acc_prev[r] ? 1 : 0) | (b->s_cur[r] << 1));
                kind[r] = (uint8_t)mmc_move_kind(chain_key(r), (uint64_t)(rng_off + step));
            }
            if (b->bar_flags && !plan.server && hi > lo) { // this thread's slice, straight into device memory
                memcpy(b->bar_flags + lo, b->h_flags + lo, (size_t)(hi - lo));
                mmc_bar_flush();
            }
            return;
        }
        for (int64_t r = lo; r < hi; r++) {
            if (acc_prev[r]) {
                b->s_cur[r] ^= s_flip; // main.jl:621
                batch_mirror_commit(b, r, prev[r]);
            }
            MoveRec &m = cur[r];
            m.mol = mol;
            m.flags = (acc_prev[r] ? 1 : 0) | (b->s_cur[r] << 1);
            batch_fill_old(b, r, m);
            const double dr = chains ? chains[r].dr_max : p->dr_max;
            const double dphi = chains ? chains[r].dphi_max : p->dphi_max;
            kind[r] = (uint8_t)propose(rng[r], dr, dphi, s.box, m.com_old, m.atoms_old, m.com_new,
                                       m.atoms_new);
        }
        (void)g;
    }

    void server_timeout_error() const
    {
        const volatile int32_t *t = b->h_timeout;
        mmc_set_error("the persistent move server timed out waiting for a control word (replica %d "
                      "at step %d saw sequence %d, low word 0x%x)", t[1], t[2], t[3], (unsigned)t[4]);
    }

    // Slow path of the result poll (any thread): has the stream died, or drained without our stamp?
    bool still_running(const Group &g)
    {
        if (status.load() != MMC_OK)
            return false;
        if (plan.server && __atomic_load_n(b->h_timeout, __ATOMIC_ACQUIRE)) {
            server_timeout_error();
            fail(MMC_ERR_HIP);
            return false;
        }
        if (plan.server && !server_async && std::chrono::steady_clock::now() - g.t_post > std::chrono::seconds(30)) {
            // e.g. a workgroup that never became resident because something else holds its
            // compute unit: give up; the epilogue posts "quit", which every workgroup honours
            // whenever it does start
            mmc_set_error("the persistent move server made no progress for 30 s (is a compute unit "
                          "per replica free?)");
            fail(MMC_ERR_HIP);
            return false;
        }
        const hipError_t q = hipStreamQuery(g.launched_on ? g.launched_on : g.stream); // (any thread: hipStreamQuery is thread-safe)
        if (q == hipErrorNotReady)
            return true;
        if (q == hipSuccess && plan.server) { // the server has ended before its run: it gave up or failed
            mmc_set_error("the persistent move server ended before the run did");
            fail(MMC_ERR_HIP);
            return false;
        }
        if (q == hipSuccess) { // drained: give the last stores a moment, then look again
            std::this_thread::sleep_for(std::chrono::milliseconds(50));
            if (drained_polls.fetch_add(1) < 40)
                return true;
            mmc_set_error("stream drained but a move result never carried stamp %u", g.stamp);
            fail(MMC_ERR_HIP);
            return false;
        }
        mmc_set_error("HIP error while waiting for a move kernel: %s", hipGetErrorString(q));
        fail(MMC_ERR_HIP);
        return false;
    }

    // ---- thread 0 only: the calls that enqueue or wait on streams ---------------------------
    int32_t read_timing(Group &g, mmc_run_stats &st)
    {
        if (g.timed) {
            float ms = 0.f;
            MMC_HIP(hipEventSynchronize(g.ev1));
            MMC_HIP(hipEventElapsedTime(&ms, g.ev0, g.ev1));
            st.kernel_ms += ms;
            st.timed_launches++;
            g.timed = false;
        }
        return MMC_OK;
    }

    int32_t launch(Group &g, int64_t step, mmc_run_stats &st, hipStream_t on = nullptr)
    {
        g.launched_on = on ? on : g.stream;
        if (plan.server) { // no launch: one control word per replica of the group
            const bool new_steps = step == 0 || (adjust && step % b->sys.n_mol == 0);
            g.n_launch++;
            g.timed = false;
            g.stamp = ++b->stamp;
            g.t_post = std::chrono::steady_clock::now();
            std::atomic_thread_fence(std::memory_order_release); // h_steps before the words
            if (b->server_stall_ms > 0 && step == 2) // test hook: a host that stops talking
                std::this_thread::sleep_for(std::chrono::milliseconds(b->server_stall_ms));
            for (int64_t r = g.r0; r < g.r0 + g.nr; r++)
                batch_server_post(b, r, step + 1, g.stamp,
                                  (unsigned)b->h_flags[r] | (new_steps ? SRV_STEPS : 0u));
            st.launches++;
            return MMC_OK;
        }
        // ev0 is recorded between the H2D copy and the kernel: ev0..ev1 brackets the kernel only
        DevGen dg{};
        if (plan.devgen) {
            const int64_t n_mol = b->sys.n_mol, i0 = step % n_mol;
            dg.seed = p->seed;
            dg.replica0 = p->replica0;
            dg.rng_off = rng_off;
            dg.step = step;
            dg.upload_steps = step == 0 || (adjust && i0 == 0);
            if (step >= g.gen_end) { // generate the next run of records (see k_propose)
                int64_t k = n_mol - 1 < 1 ? 1 : n_mol - 1;
                if (k > plan.gen_max) k = plan.gen_max;
                if (k > p->n_steps - step) k = p->n_steps - step;
                if (adjust && k > n_mol - i0) k = n_mol - i0; // step sizes change between sweeps
                dg.n_gen = (int)k;
                g.gen_end = step + k;
            }
        }
        g.n_launch++;
        // time_kernels = N: every Nth launch is bracketed by events (an event costs ~6 us of
        // stream time on its own, so N > 1 keeps the measurement from slowing what it measures)
        // (sampled from the middle of each window of N, so that N > 1 skips the first launch of a
        // call, which runs behind the burst of k_propose and with cold caches)
        g.timed = p->time_kernels > 0
                  && (g.n_launch - 1) % (unsigned)p->time_kernels == (unsigned)p->time_kernels / 2;
        g.stamp = ++b->stamp;
        DevDecide dd{};
        if (plan.devacc) { // the launch's records go to the half of d_parts of its parity
            const int64_t n_sub = std::min<int64_t>(plan.K, p->n_steps - step); // (K == 1: a step per launch)
            const int slot = (int)((step / plan.K) & 1);
            const size_t gi = (size_t)(&g - groups.data());
            dd = DevDecide{ b->d_decide, rng_off + step, b->d_parts + (size_t)slot * b->sys.R, step == 0, (int)n_sub,
                            n_sub > 1 ? b->d_queue + MMC_QUEUE_STRIDE * gi : nullptr, b->queue_base[gi] };
            if (n_sub > 1)
                b->queue_base[gi] += (unsigned)(g.nr * plan.P); // (what the launch takes: wave_ticket)
        }
        // (step > 0: a launch of this group has completed before, its proposals are outstanding)
        MMC_TRY(batch_launch(b, g.launched_on, g.r0, g.nr, plan.P, g.kernel, g.buf, step > 0, pp,
                             g.timed ? g.ev0 : nullptr, plan.devgen ? &dg : nullptr, g.stamp, plan.devacc ? &dd : nullptr));
        if (g.timed)
            MMC_HIP(hipEventRecord(g.ev1, g.launched_on));
        st.launches++;
        return MMC_OK;
    }

    // The commit of the LAST step's accepted moves (the steps before it are committed by the launch
    // that follows them).  Launch-per-step driver: every thread does its slice's bookkeeping after
    // its last Metropolis pass (settle_slice), thread 0 enqueues the group's commit kernels at once
    // (settle_enqueue) -- behind the group's last launch on its stream and beside the other group's
    // last launch -- and run_impl only waits.  (Done by the calling thread after the join this was
    // 156 us of host time per call for 65536 replicas.)
    void settle_slice(const Group &g, int64_t lo, int64_t hi)
    {
        const MoveRec *prev = b->h_moves[g.buf];
        for (int64_t r = lo; r < hi; r++) {
            b->h_accept[r] = acc_prev[r];
            if (acc_prev[r]) {
                b->s_cur[r] ^= s_flip;
                if (!plan.devgen)
                    batch_mirror_commit(b, r, prev[r]);
            }
        }
    }
    int32_t settle_enqueue(Group &g)
    {
        // (not waited for here: run_impl synchronises every group's stream once, after the last)
        return batch_settle_range(b, g.stream, g.r0, g.nr,
                                  plan.devgen ? batch_ring_slot(b, p->n_steps - 1) : b->dev_moves(g.buf), false);
    }
    // the move server applied the last accepted moves itself when it was told to quit
    void settle_server(Group &g)
    {
        for (int64_t r = g.r0; r < g.r0 + g.nr; r++)
            if (acc_prev[r])
                b->s_cur[r] ^= s_flip;
    }

    void fail(int32_t st)
    {
        int32_t ok = MMC_OK;
        if (status.compare_exchange_strong(ok, st))
            snprintf(err, sizeof(err), "%s", mmc_last_error()); // thread-local -> carry it out
    }

    // ---- the move server: every replica at its own pace ---------------------------------------
    // A chain on the server is a ping-pong between one replica's workgroups and the host; nothing
    // ties it to the other replicas.  Thread t owns the replicas [R t / T, R (t + 1) / T): it looks
    // at each in turn, and whenever one's records are in it decides, does the bookkeeping of the
    // next step and posts that replica's next control word at once.  (Stepping the replicas of a
    // group together -- collect all, decide all, post all -- made a step of 32 chains 13.8 us where
    // one chain takes 5.9; this way the chains overlap.)  Same decisions, same words per replica:
    // the chains are what they were.
    unsigned server_stamp0 = 0; // a replica's records of step s carry server_stamp0 + s + 1
    bool server_async = true;   // (the progress watchdog is this loop's own, per thread)
    void server_post_step(int64_t r, int64_t step, const RepView &v)
    {
        const bool new_steps = step == 0 || (adjust && step % b->sys.n_mol == 0);
        const int64_t k = r - v.off;
        if (step > 0 && v.acc[k])
            v.scur[k] ^= s_flip; // main.jl:621
        v.flags[k] = (uint8_t)((step > 0 && v.acc[k] ? 1 : 0) | (v.scur[k] << 1));
        v.kind[k] = (uint8_t)mmc_move_kind(chain_key(r), (uint64_t)(rng_off + step));
        std::atomic_thread_fence(std::memory_order_release); // h_steps before the word
        batch_server_post(b, r, step + 1, server_stamp0 + (unsigned)step + 1u,
                          (unsigned)v.flags[k] | (new_steps ? SRV_STEPS : 0u));
    }

    void server_thread_main(int t)
    {
        mmc_run_stats st{}; // (a copy: the threads' entries of tstats share cache lines)
        const int64_t R = b->sys.R, n_steps = p->n_steps;
        const int64_t lo = R * t / plan.T, hi = R * (t + 1) / plan.T;
        if (hi <= lo)
            return;
        const size_t n = (size_t)(hi - lo);
        std::vector<int64_t> step(n, 0);
        std::vector<int> q_done(n, 0);
        std::vector<PartOut> parts(n * plan.records());
        // this thread's slice of the per-replica arrays (see RepView); written back when it is done
        std::vector<uint8_t> l_acc(n, 0), l_kind(n, 0), l_scur(b->s_cur.begin() + lo, b->s_cur.begin() + hi),
            l_flags(n, 0);
        std::vector<double> l_energy;
        if (energies)
            l_energy.assign(energies + lo, energies + hi);
        const RepView v{ l_acc.data(), l_kind.data(), l_scur.data(), l_flags.data(),
                         energies ? l_energy.data() : nullptr, lo };
        struct WriteBack { // (on every way out)
            Driver *d; const RepView &v; int64_t lo, hi; mmc_run_stats &st; int t;
            ~WriteBack()
            {
                for (int64_t r = lo; r < hi; r++) {
                    d->acc_prev[r] = v.acc[r - lo]; d->kind[r] = v.kind[r - lo];
                    d->b->s_cur[r] = v.scur[r - lo]; d->b->h_flags[r] = v.flags[r - lo];
                    if (d->energies) d->energies[r] = v.energy[r - lo];
                }
                d->tstats[t] = st;
            }
        } write_back{ this, v, lo, hi, st, t };
        bool stalled = false;
        for (int64_t r = lo; r < hi; r++)
            server_post_step(r, 0, v);
        int64_t left = hi - lo;
        auto t_progress = std::chrono::steady_clock::now();
        for (unsigned long long spins = 1; left > 0; spins++) {
            bool any = false;
            for (int64_t r = lo; r < hi; r++) {
                int64_t &sr = step[r - lo];
                if (sr >= n_steps)
                    continue;
                const unsigned want = (server_stamp0 + (unsigned)sr + 1u) & MMC_STAMP_MASK;
                const int c = collect(r, want, &parts[(size_t)(r - lo) * plan.records()], q_done[r - lo], st);
                if (c < 0)
                    return;
                if (c == 0)
                    continue;
                decide(r, &parts[(size_t)(r - lo) * plan.records()], sr, st, v);
                q_done[r - lo] = 0;
                sr++;
                any = true;
                if (sr < n_steps) {
                    if (b->server_stall_ms > 0 && sr == 2 && !stalled) { // test hook: a host that stops talking
                        stalled = true;
                        std::this_thread::sleep_for(std::chrono::milliseconds(b->server_stall_ms));
                    }
                    server_post_step(r, sr, v);
                } else {
                    left--;
                }
            }
            if (any) {
                t_progress = std::chrono::steady_clock::now();
            } else if ((spins & 0xfffff) == 0) {
                if (std::chrono::steady_clock::now() - t_progress > std::chrono::seconds(30)) {
                    // e.g. a workgroup that never became resident because something else holds
                    // its compute unit: give up; the epilogue posts "quit", which every workgroup
                    // honours whenever it does start
                    mmc_set_error("the persistent move server made no progress for 30 s (is a compute "
                                  "unit per replica free?)");
                    fail(MMC_ERR_HIP);
                    return;
                }
                if (!still_running(groups[0]))
                    return;
            }
            if (status.load(std::memory_order_relaxed) != MMC_OK)
                return;
        }
    }

    // Device-side proposals: step 0 needs nothing from the host but the S-buffer bit of every
    // replica, so the calling thread launches it before the worker threads have their first pass
    // over the replicas behind them (~170 us in which the GPU would wait: 1.5 % of a 20-step call).
    // Host-side decisions: the FIRST group only.  The others follow by the normal path, ~150 us
    // later, and that stagger is wanted -- two launches that start together stay in step for many
    // steps (all their waves load, then all compute) and overlap badly: 1.09e8 moves/s in a 20-step
    // call with both launched at once, 1.17e8 a group at a time (round 4; all groups queued on one
    // stream here, one behind the other, was no better than this, and an event between two streams
    // cost the second launch 6 ms of host time).  Device-side decisions: see below.
    // thread_main skips the launch of step 0 for the groups launched here.
    int prelaunched = 0; // groups whose step 0 is already in flight
    mmc_run_stats pre_st{};
    void prelaunch()
    {
        if (!plan.devgen || plan.server || p->n_steps < 1)
            return;
        const int G = plan.devacc ? (int)groups.size() : 1;
        for (int gi = 0; gi < G; gi++) { // (the flag bytes of every group the kernel will decide for)
            const Group &g = groups[gi];
            for (int64_t r = g.r0; r < g.r0 + g.nr; r++)
                b->h_flags[r] = (uint8_t)(b->s_cur[r] << 1);
            if (b->bar_flags)
                memcpy(b->bar_flags + g.r0, b->h_flags + g.r0, (size_t)g.nr);
        }
        if (b->bar_flags)
            mmc_bar_flush();
        Group &g = groups[0];
        const int32_t rc = launch(g, 0, pre_st); // (the first group's; where the kernel decides the others
                                                 // follow when this one is under way: thread_main_devacc)
        if (rc != MMC_OK) {
            fail(rc);
            return;
        }
        if (trace_t.capacity() > trace_t.size())
            trace_t.push_back(now_us());
        prelaunched = 1;
    }

    // ---- device-side decisions ------------------------------------------------------------------
    // The move kernel decides (DecideConsts): a chain's next step needs nothing from the host, and
    // the host is not between two launches any more.  Every group has ONE launch in flight, K steps
    // of its chains; launches of even and odd number write the two halves of the result records in
    // turn.  Iteration (l, group): the threads do the bookkeeping of launch l - 1 from its records --
    // energies, counts, the S-buffer bit; the decisions are the record's -- and thread 0 enqueues
    // launch l, at once (one group) or when the next group's launch is half back (launch_held).
    // (With the decision on the host, a group's next launch waited for the host's pass over 32768
    // records: ~220 of the 235 us a launch takes, eight threads.)
    //
    // One stamp, one `timed` and one pair of events per group are enough, because every read of them
    // is ordered after the write it means and before the next.  Thread 0 alone writes them, in
    // launch(); all threads read g.stamp in metropolis, thread 0 reads the rest in read_timing.
    //  - Launch 0 of group 0 is written by prelaunch() before the pool starts the threads; launch 0 of
    //    the other groups by thread 0 before its first bar.wait.  Every read is behind that barrier.
    //  - Group g's stamp is read only between the two barriers of an iteration (l, g), and launch l of
    //    g is enqueued only after the second of them, where read_timing has taken launch l - 1's
    //    events.  One group: thread 0 enqueues it right there, before it reaches the first barrier of
    //    iteration (l + 1, g), behind which the next reads are.  Several groups: it is held and
    //    enqueued by launch_held() between the barriers of the NEXT group's iteration, in which the
    //    threads read that other group's stamp and nobody g's; thread 0 again arrives at the first
    //    barrier of (l + 1, g) only afterwards.  (The held launch is never the group's whose
    //    iteration it is enqueued in: it is set after one group's iteration and gone after the next.)
    //  - What a wrong stamp would do is not a hang: still_running ends every spin on a stream that
    //    has drained without the awaited stamp.
    void thread_main_devacc(int t, mmc_run_stats &st)
    {
        int sense = 0;
        const int64_t n_steps = p->n_steps;
        const int G = (int)groups.size();
        // WHEN a group's next launch is enqueued.  Its inputs are complete as soon as the records
        // of its last one are in -- but a launch enqueued then becomes ready while the OTHER
        // group's launch is still taking over the compute units, the two share them for their
        // whole length, and that costs 257 us per launch where one launch at a time, each filling
        // the tail of the one before, costs 237 (with the host's decision the host's 200 us pass
        // set that timing by accident).  So the launch waits, on the host, until `launch_at` of
        // the other group's launch in flight has come back: thread 0 looks at one record of it
        // before it starts on its own share.  (`held`: the launch that waits, -1 = none.)
        constexpr double launch_at = 0.5;
        int64_t held_step = -1;
        int held_group = -1;
        auto launch_held = [&]() {
            if (held_group < 0)
                return;
            if (status.load() == MMC_OK) {
                int32_t rc = launch(groups[held_group], held_step, st);
                if (rc != MMC_OK) fail(rc);
                if (trace_t.capacity() > trace_t.size())
                    trace_t.push_back(now_us());
            }
            held_group = -1;
        };
        const int64_t n_l = (n_steps + plan.K - 1) / plan.K; // launches per group: launch l takes steps [l K, (l + 1) K)
        // The other groups' first launches: when the first group's is under way -- its first record
        // is back, so all its workgroups are resident and working (a launch that starts while another
        // is still being dispatched shares the compute units with it for its whole length, and two
        // launches that start like that stay like that: a 20-step call took 10.0 instead of 9.0 ms,
        // in a third of the calls while a timer held the second launch back ~80 us).  It then waits
        // on the GPU for the first one's workgroups to leave.
        if (t == 0 && G > 1) {
            const Group &g0 = groups[0];
            const unsigned want = g0.stamp & MMC_STAMP_MASK;
            const PartOut *rec = &b->h_parts[g0.r0];
            for (unsigned spins = 1; part_stamp_of(*(const volatile int32_t *)&rec->ovl[1]) != want; spins++) {
                if (((spins & 0xffff) == 0 && !still_running(g0)) || status.load(std::memory_order_relaxed) != MMC_OK)
                    break;
                for (int k = 0; k < 16; k++)
                    mmc_cpu_relax();
            }
            for (int gi = 1; gi < G && status.load() == MMC_OK; gi++) {
                const int32_t rc = launch(groups[gi], 0, st);
                if (rc != MMC_OK) fail(rc);
                if (trace_t.capacity() > trace_t.size())
                    trace_t.push_back(now_us());
            }
        }
        for (int64_t l = 1; l <= n_l; l++) {
            for (int gi = 0; gi < G; gi++) {
                Group &g = groups[gi];
                bar.wait(sense); // thread 0 has enqueued launch l - 1 of this group (g.stamp is set)
                const int slot = (int)((l - 1) & 1); // (the half of the records it wrote: launch())
                const int64_t s0 = (l - 1) * plan.K;
                if (t == 0 && held_group >= 0) { // (thread 0 only knows `held`)
                    const int64_t probe = g.r0 + (int64_t)(launch_at * (double)(g.nr - 1));
                    const unsigned want = g.stamp & MMC_STAMP_MASK;
                    const PartOut *rec = &b->h_parts[(size_t)slot * b->sys.R + probe];
                    for (unsigned spins = 1; part_stamp_of(*(const volatile int32_t *)&rec->ovl[1]) != want; spins++) {
                        if (((spins & 0xffff) == 0 && !still_running(g)) || status.load(std::memory_order_relaxed) != MMC_OK)
                            break;
                        for (int k = 0; k < 16; k++)
                            mmc_cpu_relax();
                    }
                    launch_held();
                }
                if (status.load() == MMC_OK)
                    share(g, t, [&](int64_t lo, int64_t hi, bool gated) {
                        metropolis(g, lo, hi, s0, st, gated, slot);
                        if (l == n_l)
                            settle_slice(g, lo, hi);
                    });
                bar.wait(sense); // launch l - 1's records are consumed: the group's next may be enqueued
                if (t == 0) {
                    if (status.load() == MMC_OK) {
                        int32_t rc = read_timing(g, st);
                        if (rc != MMC_OK) fail(rc);
                    }
                    if (l < n_l) { // (nothing is held here: what was has been enqueued in this iteration)
                        held_group = gi;
                        held_step = l * plan.K;
                        if (G < 2) // one group: nothing to wait for
                            launch_held();
                    }
                    if (l == n_l && status.load() == MMC_OK) {
                        int32_t rc = settle_enqueue(g);
                        if (rc != MMC_OK) fail(rc);
                    }
                }
            }
        }
    }

    // Every thread runs this; slices [lo, hi) of each group belong to thread t.
    void thread_main(int t)
    {
        int sense = 0;
        if (hipSetDevice(b->sys.device) != hipSuccess)
            fail(MMC_ERR_HIP);
        if (!entry_t.empty())
            entry_t[t] = now_us();
        if (plan.server) {
            server_thread_main(t);
            return;
        }
        auto mark = [&]() {
            if (t == 0 && mark_t.capacity() > mark_t.size())
                mark_t.push_back(now_us());
        };
        mmc_run_stats st{}; // (a copy, written back on the way out: the threads' entries of tstats share cache lines)
        struct Back { mmc_run_stats &dst, &src; ~Back() { dst = src; } } back{ tstats[t], st };
        if (plan.devacc) {
            thread_main_devacc(t, st);
            return;
        }
        const int64_t n_steps = p->n_steps;
        // step s: settle step s-1's results (s > 0), propose + launch step s (s < n_steps)
        for (int64_t s = 0; s <= n_steps; s++) {
            for (Group &g : groups) {
                bar.wait(sense); // thread 0 has enqueued step s-1 of this group (g.stamp is set)
                mark();
                const bool ok = status.load() == MMC_OK;
                const int nbuf = (s == 0) ? g.buf : (g.buf ^ 1);
                if (ok)
                    share(g, t, [&](int64_t lo, int64_t hi, bool gated) {
                        if (s > 0)
                            metropolis(g, lo, hi, s - 1, st, gated);
                        if (s < n_steps)
                            proposals(g, lo, hi, s, nbuf);
                        if (s == n_steps)
                            settle_slice(g, lo, hi);
                    });
                mark();
                mark();
                bar.wait(sense); // proposals of step s are complete, results of s-1 consumed
                mark();
                if (t == 0) {
                    if (s > 0 && status.load() == MMC_OK) {
                        int32_t rc = read_timing(g, st);
                        if (rc != MMC_OK) fail(rc);
                    }
                    if (s > 0)
                        g.buf ^= 1 * (s < n_steps ? 1 : 0); // the new proposals' buffer
                    if (s == n_steps && status.load() == MMC_OK) {
                        int32_t rc = settle_enqueue(g);
                        if (rc != MMC_OK) fail(rc);
                    }
                    if (s < n_steps && status.load() == MMC_OK && !(s == 0 && (&g - groups.data()) < prelaunched)) {
                        int32_t rc = launch(g, s, st);
                        if (rc != MMC_OK) fail(rc);
                        if (trace_t.capacity() > trace_t.size())
                            trace_t.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - trace_t0).count());
                    }
                }
            }
        }
    }
};

// The driver's worker threads, kept with the batch between calls.  Creating seven threads took
// 100-190 us at the head of every call (run trace, round 4: "threads entered at 87 .. 188") -- 2 %
// of a 20-step call, and the reason the second group's pipeline slot stayed empty for the call's
// first steps.  A worker that has finished a call spins on the job counter for `block_us` (the
// next call of a run -- warm-up, then production; sweep after sweep of an NPT run -- finds it
// awake), then parks on a condition variable like an OpenMP runtime's threads after their block
// time.  One caller at a time per batch, as for every other entry point.
struct WorkerPool {
    std::vector<std::thread> th;
    std::mutex m;
    std::condition_variable cv;
    std::atomic<uint64_t> gen{ 0 };
    std::atomic<int> done{ 0 };
    Driver *job = nullptr;
    int n_active = 0;
    bool quit = false;
    int device = 0;
    int64_t block_us = 2000;

    void worker(int t)
    {
        (void)hipSetDevice(device);
        uint64_t seen = 0;
        for (;;) {
            const auto t0 = std::chrono::steady_clock::now();
            unsigned spins = 0;
            while (gen.load(std::memory_order_acquire) == seen) {
                mmc_cpu_relax();
                if ((++spins & 0xff) == 0
                    && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(block_us)) {
                    std::unique_lock<std::mutex> lk(m);
                    cv.wait(lk, [&] { return gen.load(std::memory_order_acquire) != seen || quit; });
                    break;
                }
            }
            {
                std::lock_guard<std::mutex> lk(m); // (job, n_active, quit are written under it)
                if (quit)
                    return;
                seen = gen.load(std::memory_order_acquire);
            }
            if (t < n_active)
                job->thread_main(t);
            done.fetch_add(1, std::memory_order_release);
        }
    }
    // thread_main(0) on the calling thread, thread_main(1 .. T-1) on workers; returns when all have
    void run(Driver *d, int T)
    {
        while ((int)th.size() < T - 1) {
            const int t = (int)th.size() + 1;
            th.emplace_back([this, t] { worker(t); });
        }
        {
            std::lock_guard<std::mutex> lk(m);
            job = d;
            n_active = T;
            done.store(0, std::memory_order_relaxed);
            gen.fetch_add(1, std::memory_order_release);
        }
        cv.notify_all();
        d->thread_main(0);
        while (done.load(std::memory_order_acquire) < (int)th.size())
            mmc_cpu_relax();
    }
    static void destroy(void *p)
    {
        WorkerPool *w = static_cast<WorkerPool *>(p);
        {
            std::lock_guard<std::mutex> lk(w->m);
            w->quit = true;
            w->gen.fetch_add(1, std::memory_order_release);
        }
        w->cv.notify_all();
        for (auto &x : w->th)
            x.join();
        delete w;
    }
};

} // namespace

// What the call will do (RunPlan), from the batch's options and the call's parameters alone: no HIP
// call, no allocation, nothing written into *b.  Every requirement on the shape of a call is here.
static int32_t run_plan(const mmc_batch *b, const mmc_run_params *p, bool chains, int adjust, RunPlan *out)
{
    const DeviceSystem &s = b->sys;
    const int64_t R = s.R;
    const bool wolf = b->coulomb_style == MMC_COULOMB_WOLF;
    RunPlan pl;
    MMC_REQUIRE(!b->quat_mode || b->device_moves, MMC_ERR_UNSUPPORTED,
                "orientations are set (mmc_batch_set_orientations): the quaternion move generation "
                "runs on the device only, set option device_moves = 1");
    pl.G = p->n_groups < 1 ? 1 : p->n_groups;
    if (pl.G > R) pl.G = (int)R;
    if (pl.G > MMC_MAX_GROUPS) pl.G = MMC_MAX_GROUPS;
    if (p->n_steps == 0) { // (nothing will run: nothing more is asked of the call)
        *out = pl;
        return MMC_OK;
    }
    pl.devgen = b->device_moves != 0;
    // A fixed solute: its record is k_solute_move's, beside a launch per step whose decision the host
    // makes.  The move server and the latency form have no such launch: refused where asked for by
    // name, not taken where the size would choose them; "accept_on_device", "steps_per_launch" and
    // "whole_call" fall back as they do wherever they do not apply.
    pl.solute = b->sol.n > 0;
    MMC_REQUIRE(!pl.solute || (b->persistent != 1 && b->kernel != 4), MMC_ERR_UNSUPPORTED,
                "a solute is set (mmc_batch_set_solute): the persistent move server (option persistent = 1) and "
                "kernel 4 do not evaluate it");
    pl.P = p->n_parts > 0 ? p->n_parts : b->n_parts;
    if (b->kernel == 4) { // parts are waves, four to a workgroup; the host sees one record per workgroup
        if (p->n_parts <= 0) { // sixteen, or as many as the system's size asks for
            pl.P = 16;
            while (pl.P < LAT_MAX_PARTS && !lat_applies(pl.P, (int)s.n_mol, (int)s.nkvecs))
                pl.P += LAT_WAVES;
        }
        MMC_REQUIRE(lat_applies(pl.P, (int)s.n_mol, (int)s.nkvecs), MMC_ERR_UNSUPPORTED,
                    "kernel 4 needs n_parts = 4, 8, ... %d with at most %d molecules per pair part",
                    LAT_MAX_PARTS, LAT_MAXMOL);
        pl.P /= LAT_WAVES;
    } else if (pl.P > MMC_MAX_PARTS) {
        pl.P = MMC_MAX_PARTS;
    }
    MMC_REQUIRE(!s.pb.on || pl.devgen, MMC_ERR_UNSUPPORTED,
                "per-replica boxes: the trial moves are drawn on the device (device_moves = 1)");
    if (b->persistent != 0 && !s.pb.on && !wolf && !pl.solute) { // small batches: the persistent move server (one box, Ewald style)
        pl.server = batch_server_applies(b) && (b->persistent == 1 || R <= MMC_SERVER_AUTO_MAX);
        MMC_REQUIRE(pl.server || b->persistent != 1, MMC_ERR_UNSUPPORTED,
                    "the persistent move server needs device_moves = 1, the table kernel, no "
                    "orientations and at most one replica per compute unit");
        if (pl.server) { // the parts are waves of one workgroup: the host sees one record
            pl.server_waves = p->n_parts > 1 ? (p->n_parts > SRV_WAVES ? SRV_WAVES : p->n_parts)
                                             : batch_server_parts(s.n_mol, R);
            pl.P = 1;
            // few replicas: the latency server, several workgroups per replica, one record each
            int wgs = batch_lat_shape(b);
            if (p->n_parts > 1 && b->server_wgs != 0) { // an explicit part count picks the shape
                wgs = (p->n_parts % LAT_WAVES == 0 && lat_applies(p->n_parts, (int)s.n_mol, (int)s.nkvecs)
                       && R * (p->n_parts / LAT_WAVES) <= (int64_t)b->n_cus && b->kernel == 4)
                          ? p->n_parts / LAT_WAVES : (b->kernel == 4 ? -1 : 0);
                MMC_REQUIRE(wgs >= 0, MMC_ERR_UNSUPPORTED,
                            "kernel 4 with the move server needs n_parts = 8, 12, ... %d (a multiple of 4 whose "
                            "pair parts hold at most %d molecules each)", LAT_MAX_PARTS, LAT_MAXMOL);
            }
            if (wgs >= 2) {
                pl.server_lat_wgs = wgs;
                pl.server_waves = LAT_WAVES * wgs;
                pl.P = wgs;
            }
        }
    }
    pl.T = p->n_threads > 0 ? p->n_threads : 1;
    if (pl.T > 64) pl.T = 64;
    // Streams.  Host proposals: one stream per group, so that a group's H2D copy of its move
    // records overlaps the other group's kernel.  Device proposals: nothing but a flag byte
    // per replica is copied; the groups alternate between TWO streams, so that the start of
    // one launch -- 5120 waves that all load their move record, then all build phase tables,
    // ... in step -- overlaps the end of the other, whose waves have long drifted apart:
    // 1.30e8 moves/s against 1.22e8 with every launch alone on the GPU (65536 chains of 750
    // molecules, round 4).  A launch's own span then says less than its cost: see
    // mmc_run_stats.kernel_ms.  (p->n_streams overrides.)
    pl.n_streams = p->n_streams > 0 ? p->n_streams : (pl.devgen ? (pl.G < 2 ? pl.G : 2) : pl.G);
    // Who decides: the move kernel itself where it holds the whole move (one part, the wave kernel)
    // and draws it (device-side proposals); the host otherwise -- parts that only the host adds up,
    // the caller's proposals, the move server, and chains whose step sizes the host adapts between
    // sweeps (the launches are enqueued a step ahead of the host's bookkeeping).
    pl.devacc = pl.devgen && !pl.server && pl.P == 1 && !b->zero_copy_moves && !(chains && adjust) && !pl.solute;
    int64_t nr_max = 0;
    for (int g = 0; g < pl.G; g++) {
        auto &pg = pl.group[g];
        pg.r0 = R * g / pl.G;
        pg.nr = R * (g + 1) / pl.G - pg.r0;
        pg.kernel = batch_kernel_for(b, pg.nr, pl.P);
        pl.devacc = pl.devacc && pg.kernel == 2;
        pl.cand = pl.cand || (!pl.server && pl.P == 1 && pg.kernel == 2);
        nr_max = std::max(nr_max, pg.nr);
    }
    // ... and how many steps a launch takes: one record per replica and launch then, so only where
    // the caller asked for energies and counts (no per-chain averages, no trace of single steps),
    // and where a burst of device-made proposals covers them (n_mol > MMC_GEN_MAX).
    const bool multi_ok = !chains && b->trace_steps == 0 && s.n_mol > MMC_GEN_MAX;
    // by size (option "accept_on_device" < 0): where a launch can take several steps the kernel
    // decides; for one step per launch only where a thread's pass over more than 4096 records would
    // outlast the launch
    const int want = b->accept_on_device >= 0 ? b->accept_on_device
                                              : ((multi_ok && b->steps_per_launch != 1) || nr_max > (int64_t)4096 * pl.T);
    pl.devacc = pl.devacc && want == 1;
    if (pl.devacc && multi_ok) {
        pl.K = b->steps_per_launch > 0 ? b->steps_per_launch : 8;
        if (pl.K != 1 && pl.K != 2 && pl.K != 4 && pl.K != 8 && pl.K != 16)
            pl.K = 1;
        // A whole call in ONE launch per group (option "whole_call" = 1): K = the call's steps, as
        // many as a record carries and a burst of proposals may draw (n_mol - 1; the ring grows to
        // hold them).  Not taken by default: at the bench's 20-step call it ran 1.34 x 10^8 moves/s
        // against 1.40 for launches of eight, both with the queue of units (profiles/README.md,
        // "The 20-step call") -- one launch's tail is a whole 20-step unit long, and nothing covers it.
        if (b->whole_call == 1) {
            pl.K = (int)std::min<int64_t>(std::min<int64_t>(p->n_steps, MMC_STEPS_PER_LAUNCH_MAX), s.n_mol - 1);
            pl.gen_max = std::max(pl.K, (int)MMC_GEN_MAX);
        }
    }
    pl.no_tail_share = !pl.devacc;
    *out = pl;
    return MMC_OK;
}

// Everything of a call that touches the device before its first launch, in this order: the step sizes
// and the ring (or the host mirror), streams and events, what the kernel's own decision reads, the
// candidate lists, the move server; then the driver's own arrays and the worker pool.
static int32_t run_prepare(Driver &d)
{
    mmc_batch *b = d.b;
    const mmc_run_params *p = d.p;
    const RunPlan &pl = d.plan;
    DeviceSystem &s = b->sys;
    const int64_t R = s.R;
    if (pl.devgen) {
        for (int64_t r = 0; r < R; r++)
            b->h_steps[r] = d.chains ? make_double2(d.chains[r].dr_max, d.chains[r].dphi_max)
                                     : make_double2(p->dr_max, p->dphi_max);
        b->mirror_valid = false; // the host copy of the coordinates is not maintained
        MMC_TRY(batch_ensure_ring(b));
    } else
        MMC_TRY(batch_refresh_mirror(b));
    d.bar.n = pl.T;
    d.pp = mmc_pair_params(b->lj_rcut, b->qq_rcut, 0.0, 0.5, s.bv.kappa, false);
    d.groups.resize(pl.G);
    for (int g = 0; g < pl.G; g++) {
        Group &dg = d.groups[g];
        dg.r0 = pl.group[g].r0;
        dg.nr = pl.group[g].nr;
        dg.kernel = pl.group[g].kernel;
        // streams and events live as long as the batch: creating and destroying them costs ~3 ms
        // per call, a fifth of a 20-step run
        if (g >= pl.n_streams) {
            dg.stream = d.groups[g % pl.n_streams].stream;
        } else {
            if (!b->run_streams[g])
                MMC_HIP(hipStreamCreateWithFlags(&b->run_streams[g], hipStreamNonBlocking));
            dg.stream = b->run_streams[g];
        }
        if (p->time_kernels) {
            for (int k = 0; k < 2; k++)
                if (!b->run_events[g][k])
                    MMC_HIP(hipEventCreate(&b->run_events[g][k]));
            dg.ev0 = b->run_events[g][0];
            dg.ev1 = b->run_events[g][1];
        }
    }
    if (pl.devacc) {
        MMC_TRY(batch_ensure_ring(b, pl.gen_max + 2));
        DecideConsts dc{};
        dc.temperature = p->temperature; dc.factor = s.bv.factor;
        dc.seed = p->seed; dc.replica0 = (uint32_t)p->replica0;
        dc.flags = b->d_flags;
        dc.temps = d.temps ? b->d_temps : nullptr; // (part of the memcmp below: switching the ladder on or off uploads again)
        dc.ring = b->d_ring; dc.ring_slots = b->ring_slots; dc.ring_stride = s.R;
        if (!b->d_decide)
            MMC_TRY(s.dmalloc((void **)&b->d_decide, sizeof(DecideConsts)));
        if (!b->d_queue || b->queue_reset) { // (zero tickets taken: every group's count starts again)
            if (!b->d_queue)
                MMC_TRY(s.dmalloc((void **)&b->d_queue, sizeof(unsigned) * MMC_QUEUE_STRIDE * MMC_MAX_GROUPS));
            MMC_HIP(hipMemset(b->d_queue, 0, sizeof(unsigned) * MMC_QUEUE_STRIDE * MMC_MAX_GROUPS));
            MMC_HIP(hipDeviceSynchronize()); // (the driver's streams do not wait for the null stream)
            memset(b->queue_base, 0, sizeof(b->queue_base));
            b->queue_reset = false;
        }
        if (memcmp(&dc, &b->decide_host, sizeof(dc)) != 0) { // (the same from call to call of a run)
            MMC_HIP(hipMemcpy(b->d_decide, &dc, sizeof(dc), hipMemcpyHostToDevice));
            b->decide_host = dc;
        }
    }
    if (pl.cand)
        MMC_TRY(batch_cand_prepare(b, d.pp));
    if (pl.server) { // the one kernel runs on the first group's stream: that is the stream to watch
        for (Group &g : d.groups)
            g.stream = d.groups[0].stream;
        MMC_TRY(batch_server_start(b, d.groups[0].stream, pl.server_waves, d.pp, p->seed, p->replica0,
                                   b->steps_done, pl.server_lat_wgs));
    }
    d.rng.resize(pl.devgen ? 0 : R); // (device-side proposals draw everything from Philox counters)
    for (int64_t r = 0; r < (pl.devgen ? 0 : R); r++) { // hash of (seed, global replica index, steps already run)
        uint64_t h = p->seed;
        h = Rng::splitmix(h) ^ (p->replica0 + (uint64_t)r);
        h = Rng::splitmix(h) ^ (uint64_t)b->steps_done;
        d.rng[r].seed(h);
    }
    d.acc_prev.assign(R, 0);
    d.kind.assign(R, 0);
    b->trace_delta.assign((size_t)(b->trace_steps * R), 0.0);
    b->trace_flags.assign((size_t)(b->trace_steps * R), 0);
    d.tstats.assign(pl.T, mmc_run_stats{});
    if (pl.server) { // one stamp per step, the same sequence for every replica (Driver::server_post_step)
        d.server_stamp0 = b->stamp;
        b->stamp += (unsigned)p->n_steps;
    }
    if (!b->pool) { // (the first call pays for it)
        WorkerPool *w = new WorkerPool();
        w->device = s.device;
        if (const char *e = getenv("MMC_POOL_BLOCKTIME_US"))
            w->block_us = atoll(e);
        b->pool = w;
        b->pool_destroy = &WorkerPool::destroy;
    }
    return MMC_OK;
}

static int32_t run_impl(mmc_batch *b, const mmc_run_params *p, double *energies,
                        mmc_chain *chains, int32_t adjust, mmc_run_stats *stats)
{
    BATCH_CHECK(b);
    BATCH_USABLE(b);
    BATCH_NO_VOLUME_TRIAL(b);
    MMC_REQUIRE(p && (energies || chains) && stats, MMC_ERR_ARG, "NULL argument");
    MMC_REQUIRE(!b->has_prev, MMC_ERR_STATE, "proposals outstanding: call mmc_batch_settle first");
    MMC_REQUIRE(p->temperature > 0 && p->n_steps >= 0, MMC_ERR_ARG, "bad run parameters");
    BATCH_S_FRESH(b, "mmc_batch_run");
    memset(stats, 0, sizeof(*stats));
    // ---- 1. what the call will do ----
    RunPlan plan;
    MMC_TRY(run_plan(b, p, chains != nullptr, adjust, &plan));
    if (p->n_steps == 0)
        return MMC_OK;
    const int64_t R = b->sys.R;

    // ---- 2. everything it needs on the device and the host, before the first launch ----
    Driver d(plan);
    d.b = b; d.p = p; d.energies = energies; d.chains = chains; d.adjust = adjust;
    d.temps = b->temps.empty() ? nullptr : b->temps.data();
    d.s_flip = b->coulomb_style == MMC_COULOMB_WOLF ? 0 : 1;
    d.rng_off = b->steps_done;
    d.inject_left.store(b->inject_torn);
    MMC_TRY(run_prepare(d));

    const auto t0 = std::chrono::steady_clock::now();
    const bool run_trace = getenv("MMC_RUN_TRACE") != nullptr; // (developer: where a call's fixed cost goes)
    const auto t_enter = t0;
    if (run_trace) {
        d.trace_t.reserve(64);
        d.trace_t0 = t0;
        d.entry_t.assign(plan.T, 0.0);
        d.mark_t.reserve(4 * 12);
    }
    // ---- 3. the run: the first launch from this thread, then the threads ----
    d.prelaunch();
    static_cast<WorkerPool *>(b->pool)->run(&d, plan.T);
    // ---- 4. finish: release the server, wait for the last commits, add up, leave the batch's state right ----
    const auto t_join = std::chrono::steady_clock::now();
    if (plan.server) { // release the server whatever happened: last accept decisions + quit
        for (int64_t r = 0; r < R; r++)
            batch_server_post(b, r, p->n_steps + 1, 0u,
                              SRV_QUIT | (d.status.load() == MMC_OK && d.acc_prev[r] ? SRV_ACCEPT : 0u));
        const hipError_t e = hipStreamSynchronize(d.groups[0].stream);
        if (e != hipSuccess) {
            mmc_set_error("the persistent move server failed: %s", hipGetErrorString(e));
            d.fail(MMC_ERR_HIP);
        }
#ifdef SRV_PROFILE // diagnostic build: how long each wave of replica 0 spent in its unit per step
        else {
            const int32_t *t = b->h_timeout;
            fprintf(stderr, "server profile, unit of wave 0..7 (10 ns ticks / step):");
            for (int q = 0; q < 8; q++)
                fprintf(stderr, " %.1f", t[8 + q] / (double)p->n_steps);
            fprintf(stderr, "\n");
        }
#endif
        if (e == hipSuccess && __atomic_load_n(b->h_timeout, __ATOMIC_ACQUIRE)) {
            d.server_timeout_error();
            d.fail(MMC_ERR_HIP);
        }
    }
    int32_t status = d.status.load();
    auto t_enq = t_join;
    if (status == MMC_OK) { // (the commit of the last proposals is already enqueued: Driver::settle_enqueue)
        if (plan.server)
            for (Group &g : d.groups)
                d.settle_server(g);
        t_enq = std::chrono::steady_clock::now();
    } else
        mmc_set_error("%s", d.err);
    for (size_t g = 0; g < d.groups.size(); g++) // the commits of all groups, waited for once
        if (d.groups[g].stream) {
            const hipError_t e = hipStreamSynchronize(d.groups[g].stream);
            if (e != hipSuccess && status == MMC_OK) {
                mmc_set_error("hipStreamSynchronize failed after the last commit: %s", hipGetErrorString(e));
                status = MMC_ERR_HIP;
            }
        }
    const auto t1 = std::chrono::steady_clock::now();

    d.tstats.push_back(d.pre_st);
    for (const mmc_run_stats &w : d.tstats) {
        stats->moves += w.moves; stats->launches += w.launches;
        stats->trans_attempt += w.trans_attempt; stats->trans_accept += w.trans_accept;
        stats->rot_attempt += w.rot_attempt; stats->rot_accept += w.rot_accept;
        stats->overlaps += w.overlaps; stats->kernel_ms += w.kernel_ms;
        stats->timed_launches += w.timed_launches;
        stats->torn_records += w.torn_records;
    }
    stats->server_steps = plan.server ? p->n_steps : 0;
    stats->device_decisions = plan.devacc ? stats->moves : 0;
    if (plan.server) // control words are posted per replica as it goes: count what a lock-step driver would
        stats->launches = p->n_steps * (int64_t)d.groups.size();
    stats->wall_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    for (int64_t r = 0; r < R; r++)
        stats->energy_sum += chains ? chains[r].energy : energies[r];
    for (size_t g = 0; g < d.groups.size(); g++) // (the streams stay with the batch)
        if (d.groups[g].stream)
            (void)hipStreamSynchronize(d.groups[g].stream);
    if (run_trace) {
        const auto t2 = std::chrono::steady_clock::now();
        auto us = [](std::chrono::steady_clock::duration x) { return std::chrono::duration<double, std::micro>(x).count(); };
        fprintf(stderr, "run trace: threads %.0f us, final settle %.0f us (enqueued after %.0f), last sync %.0f us; launches at",
                us(t_join - t_enter), us(t1 - t_join), us(t_enq - t_join), us(t2 - t1));
        for (double x : d.trace_t)
            fprintf(stderr, " %.0f", x);
        fprintf(stderr, "\nrun trace: threads entered at");
        for (double x : d.entry_t)
            fprintf(stderr, " %.0f", x);
        fprintf(stderr, "\nrun trace: thread 0 per (step, group) [after barrier, after its share, (same), after barrier]:");
        for (size_t k = 0; k < d.mark_t.size(); k++)
            fprintf(stderr, "%s%.0f", k % 4 == 0 ? " | " : " ", d.mark_t[k]);
        fprintf(stderr, "\n");
    }
    b->buf = 0;
    b->has_prev = false;
    b->inject_torn = 0;
    if (status == MMC_OK)
        b->steps_done += p->n_steps;
    else { // accepted moves, S-buffer parity and the caller's energies may disagree now
        b->needs_reload = true;
        b->cand.dirty = true;
        b->queue_reset = true;
        b->reloaded.assign(R, 0);
    }
    return status;
}

extern "C" int32_t mmc_batch_run(mmc_batch *b, const mmc_run_params *p, double *energies,
                                 mmc_run_stats *stats)
{
    MMC_REQUIRE(energies, MMC_ERR_ARG, "NULL argument");
    return run_impl(b, p, energies, nullptr, 0, stats);
}

extern "C" int32_t mmc_batch_run_chains(mmc_batch *b, const mmc_run_params *p, mmc_chain *chains,
                                        int32_t adjust, mmc_run_stats *stats)
{
    MMC_REQUIRE(chains, MMC_ERR_ARG, "NULL argument");
    if (b)
        BATCH_ONE_BOX(b, "mmc_batch_run_chains");
    if (b)
        for (int64_t r = 0; r < b->sys.R; r++)
            MMC_REQUIRE(chains[r].dr_max >= 0 && chains[r].dphi_max >= 0
                            && (!adjust || (chains[r].trans_set_value > 0 && chains[r].rot_set_value > 0)),
                        MMC_ERR_ARG, "chain %lld: bad step sizes / set values", (long long)r);
    return run_impl(b, p, nullptr, chains, adjust, stats);
}

// An NPT chain of a one-replica batch (include/mmc_hip.h; Ewald/volumeChange.jl:59-147): sweeps of
// trial moves on the batch's own driver -- at 10 000 molecules the latency move server, 21
// workgroups -- each followed by one volume move on the same device state.
extern "C" int32_t mmc_batch_run_npt(mmc_batch *b, const mmc_run_params *p, const mmc_npt_params *q,
                                     double *energy, mmc_run_stats *stats, mmc_npt_stats *ns)
{
    BATCH_CHECK(b);
    BATCH_NOT_WOLF(b, "mmc_batch_run_npt");
    BATCH_NO_SOLUTE(b, "mmc_batch_run_npt");
    BATCH_ONE_BOX(b, "mmc_batch_run_npt (per-replica boxes: mmc_batch_run_npt_replicas)");
    MMC_REQUIRE(p && q && energy && stats && ns, MMC_ERR_ARG, "NULL argument");
    MMC_REQUIRE(b->sys.R == 1, MMC_ERR_UNSUPPORTED,
                "a batch has one box: an NPT chain needs a batch of ONE replica");
    MMC_REQUIRE(b->temps.empty(), MMC_ERR_UNSUPPORTED,
                "mmc_batch_run_npt: per-replica temperatures are set (mmc_batch_set_temperatures); a ladder "
                "of NPT chains is mmc_batch_run_npt_replicas");
    MMC_REQUIRE(q->n_sweeps >= 0 && q->moves_per_sweep >= 0 && q->vmax >= 0 && q->alpha > 0
                    && p->temperature > 0, MMC_ERR_ARG, "bad NPT parameters");
    memset(stats, 0, sizeof(*stats));
    memset(ns, 0, sizeof(*ns));
    DeviceSystem &s = b->sys;
    const int64_t n_mol = s.n_mol;
    const double beta = 1.0 / p->temperature;
    mmc_run_params pp = *p;
    pp.n_steps = q->moves_per_sweep > 0 ? q->moves_per_sweep : n_mol;
    const ChainKey ck{ p->seed, (uint32_t)p->replica0 };
    for (int64_t sweep = 0; sweep < q->n_sweeps; sweep++) {
        mmc_run_stats st;
        MMC_TRY(run_impl(b, &pp, energy, nullptr, 0, &st));
        stats->moves += st.moves; stats->launches += st.launches;
        stats->trans_attempt += st.trans_attempt; stats->trans_accept += st.trans_accept;
        stats->rot_attempt += st.rot_attempt; stats->rot_accept += st.rot_accept;
        stats->overlaps += st.overlaps; stats->kernel_ms += st.kernel_ms;
        stats->timed_launches += st.timed_launches; stats->torn_records += st.torn_records;
        stats->server_steps += st.server_steps; stats->wall_ms += st.wall_ms;
        stats->device_decisions += st.device_decisions;
        // ---- the volume move ----
        const auto t0 = std::chrono::steady_clock::now();
        const Uniform2 u = mmc_draw(ck, (uint64_t)b->steps_done, MMC_SLOT_VOLUME);
        const double box = s.box, vol_old = box * box * box;
        const double vol_new = vol_old + (u.a - 0.5) * q->vmax;          // volumeChange.jl:59
        ns->vol_attempt++;
        bool accepted = false;
        if (vol_new > 0.0) {
            const double L_new = cbrt(vol_new);                          // :60
            if (b->lj_rcut <= L_new / 2 && b->qq_rcut <= L_new / 2) {    // (else: minimum image would break)
                mmc_totals tot;
                MMC_TRY(mmc_batch_volume_trial(b, L_new, q->alpha / L_new, &tot));
                const double arg = -beta * (q->pressure * (vol_new - vol_old)
                                            - (double)n_mol * log(vol_new / vol_old) / beta
                                            + (tot.energy - *energy));   // :129-130
                accepted = u.b < exp(arg < 700.0 ? arg : 700.0);         // :132
                if (accepted) {
                    MMC_TRY(mmc_batch_volume_accept(b));
                    *energy = tot.energy;
                } else {
                    MMC_TRY(mmc_batch_volume_reject(b));
                }
            }
        }
        ns->vol_accept += accepted;
        ns->volume_sum += s.box * s.box * s.box;
        ns->volume_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    ns->box = s.box;
    stats->energy_sum = *energy;
    return MMC_OK;
}

// Test hook (option "trace_steps" = N): dU = d_lj + d_real + d_recip and the decision (bit 0
// accepted, bit 1 overlap, bit 2 rotation) of the first N steps of every replica of the last run.
extern "C" int32_t mmc_batch_get_trace(mmc_batch *b, double *delta, uint8_t *flags)
{
    MMC_REQUIRE(b && delta && flags, MMC_ERR_ARG, "NULL argument");
    memcpy(delta, b->trace_delta.data(), sizeof(double) * b->trace_delta.size());
    memcpy(flags, b->trace_flags.data(), b->trace_flags.size());
    return MMC_OK;
}

extern "C" int32_t mmc_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
    MMC_REQUIRE(ctr && key && out, MMC_ERR_ARG, "NULL argument");
    const Philox x = philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
    for (int k = 0; k < 4; k++)
        out[k] = x.v[k];
    return MMC_OK;
}

// main.jl:667-679
extern "C" int32_t mmc_chain_block_line(const mmc_chain *c, int64_t block, int64_t n_mol, double box,
                                        double ideal_term, char *buf, int64_t len)
{
    MMC_REQUIRE(c && buf && len > 0 && n_mol > 0 && box > 0, MMC_ERR_ARG, "bad argument");
    const double energy = c->avg_energy / (double)c->steps_taken / (double)n_mol;
    const double rt = (double)c->trans_naccept / (double)c->trans_attempt;
    const double rr = (double)c->rot_naccept / (double)c->rot_attempt;
    const int n = snprintf(buf, (size_t)len,
                           "Block: %4lld, Energy: %8.2f, Ratio trans: %4.2f, dr_max: %4.2f, Ratio rot: "
                           "%4.2f, d\xcf\x95_max: %4.2f, instant energy: %8.2f, overlap count: %4lld, "
                           "pressure: %8.2f",
                           (long long)block, energy, rt, c->dr_max, rr, c->dphi_max,
                           c->energy / (double)n_mol, (long long)c->overlaps,
                           ideal_term + c->virial / box / box / box);
    MMC_REQUIRE(n >= 0 && n < len, MMC_ERR_ARG, "block line needs %d bytes, buffer has %lld", n + 1,
                (long long)len);
    return MMC_OK;
}
