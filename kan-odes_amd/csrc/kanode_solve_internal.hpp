// kanode_solve_internal.hpp — what the integrator's translation units share (kanode_solve.cpp: the forward
// drivers; kanode_adjoint.cpp: the InterpolatingAdjoint; kanode_train.cpp: forward sensitivities and the
// device-resident training loops): the solution object, the Tsit5 tableau, the error macros, the mapped
// step-control helpers, the staged uploads and the fragments every driver states the same way.
// C++ linkage, host only, not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <string>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <type_traits>
#include <vector>

#include "kan_adjloop.hpp"
#include "kan_buf.hpp"
#include "kan_kernels.hpp"
#include "kanode.h"
#include "kanode_internal.hpp"

// Tsitouras 5(4) (OrdinaryDiffEq tsit_tableaus.jl)
constexpr double TC[6] = {0.161, 0.327, 0.9, 0.9800255409045097, 1.0, 1.0};
constexpr double TA[6][6] = {
    {0.161, 0, 0, 0, 0, 0},
    {-0.008480655492356989, 0.335480655492357, 0, 0, 0, 0},
    {2.897153057105493, -6.359448489975075, 4.3622954328695815, 0, 0, 0},
    {5.325864828439257, -11.748883564062828, 7.4955393428898365, -0.09249506636175525, 0, 0},
    {5.86145544294642, -12.92096931784711, 8.159367898576159, -0.071584973281401, -0.028269050394068383, 0},
    {0.09646076681806523, 0.01, 0.4798896504144996, 1.379008574103742, -3.290069515436081, 2.324710524099774},
};
constexpr double BT[7] = {-0.00178001105222577714, -0.0008164344596567469, 0.007880878010261995,
                          -0.1447110071732629,     0.5823571654525552,     -0.45808210592918697,
                          0.015151515151515152};
// dense output b_i(θ) = Σ_m RI[i][m] θ^(m+1)  (Tsit5Interp)
constexpr double RI[7][4] = {
    {1.0, -2.763706197274826, 2.9132554618219126, -1.0530884977290216},
    {0.0, 0.13169999999999998, -0.2234, 0.1017},
    {0.0, 3.9302962368947516, -5.941033872131505, 2.490627285651253},
    {0.0, -12.411077166933676, 30.33818863028232, -16.548102889244902},
    {0.0, 37.50931341651104, -88.1789048947664, 47.37952196281928},
    {0.0, -27.896526289197286, 65.09189467479366, -34.87065786149661},
    {0.0, 1.5, -4.0, 2.5},
};

inline void interp_weights(double theta, double w[7]) {
    for (int i = 0; i < 7; ++i) {
        double s = 0.0;
        for (int m = 0; m < 4; ++m) s += RI[i][m] * std::pow(theta, (double)(m + 1));
        w[i] = s;
    }
}

inline kanode_solver_options resolved(const kanode_solver_options* o) {
    kanode_solver_options d;
    kanode_solver_options_default(&d);
    return o ? *o : d;
}

// Dense output: step n keeps u_n and k_2..k_7 in slot n (7 states); k_1 of step n is
// k_7 of step n-1 (FSAL), k_1 of step 0 has its own buffer.  Without recording only
// two slots are used, alternately.
// device / pinned scalar slots of a solution: 8 norm totals, then an adaptive adjoint step's finish
// terms at 8 (the FK step: 1 + P <= 34) or its <= kAdjFinishBlocks partials at 16
constexpr int kScalars = 16 + kan::kAdjFinishBlocks + 16;

struct kanode_solution {
    kanode_handle* h = nullptr;
    int dtype = 0;
    size_t esize = 8;
    int64_t n = 0;                   // elements of one state (N·B)
    int64_t batch = 0;
    double t0 = 0, tf = 0;
    std::vector<double> saveat;
    std::vector<double> ts, dts;     // accepted steps: start time, step
    std::vector<void*> slots;
    bool slots_borrowed = false;     // slots point into fused.block (one-workgroup solve), not owned
    bool qform = false;              // slots hold u_n, Q_1..Q_4, k_7 (fk_step_pp_wave_kernel) instead of u_n, k_2..k_7
    kan::DevBuf k1_0_buf;
    void* k1_0() const { return k1_0_buf.ptr(); }
    bool record = true;
    // one-workgroup small-chain solve (kd_chain_tsit5_kernel): contiguous dense output and the
    // device copies of saveat, step times and the result block
    struct Fused {
        kan::DevBuf block;                 // cap steps of 7 states
        kan::DevBuf saveat;
        kan::DevBuf ts;                    // [ts_cap] then dts [ts_cap] (read at the block's cap)
        kan::MappedBuf hts;                // pinned host staging of ts | dts; kernels write its device address (null: copied)
        kan::DevBuf out;                   // naccept, nreject, nf, status
        kan::DevBuf adj_meta;              // adjoint: stops, jump rows and offsets
        kan::PinnedBuf hup;                // pinned staging of the small uploads (staged_upload)
        hipEvent_t hup_ev = nullptr;       // recorded after the last upload from hup
        bool hup_pending = false;
        // the bytes last uploaded into saveat / adj_meta: a training loop passes the same saveat and stops every
        // iteration, and an unchanged upload is skipped (each one is a copy launch on the stream's critical path)
        std::vector<char> saveat_last, meta_last;
        int64_t cap(size_t sb) const { return (int64_t)(block.bytes() / (7 * sb)); }   // steps the block holds
        int64_t ts_cap() const { return (int64_t)(ts.bytes() / (2 * sizeof(double))); }
        double* dts(size_t sb) const { return ts.as<double>() + cap(sb); }
    } fused;
    kan::DevBuf dscal_buf;           // device scalars (norm totals; an adaptive FK adjoint step's 1 + P terms)
    // their pinned host mirror (mapped, coherent).  The host-controlled adaptive loops have their step-control
    // scalars written to its device address (mscal) by the producing kernels, so reading them costs a stream
    // synchronisation and no copy launch (a D2H hipMemcpyAsync of 8 bytes ran as a ~4.4 us blit kernel, twice
    // per FK training step).  mscal is null if the runtime gave no device address: those loops then copy from
    // dscal as before.
    kan::MappedBuf hscal_buf;
    // mapped, coherent pinned host memory for a step's per-block error partials (the FK step path: the
    // host sums them, so no final-reduction launch per adaptive step); hparts / its device address mparts
    kan::MappedBuf hparts_buf;
    double* dscal() const { return dscal_buf.as<double>(); }
    double* hscal() const { return hscal_buf.as<double>(); }
    double* mscal() const { return hscal_buf.dev<double>(); }
    double* hparts() const { return hparts_buf.as<double>(); }
    double* mparts() const { return hparts_buf.dev<double>(); }
    // a call on this solution failed: its kernels may still be in flight and its mapped step-control slots
    // may hold written values; the next call drains the stream and re-arms every slot first (ctl_begin)
    bool ctl_dirty = false;
    // the persistent pair adjoint's device buffer: [arrival counter, abort word][slot table | ts | dts][exchange slots]
    kan::DevBuf padj;
    kan::DevBuf hs_dev;              // KANODE_OPT_RECORD_ADJOINT_STEPS: the one-launch adjoints' step sizes
    // the device-controlled Fisher-KPP solve (solve_fk_loop): its state and host mirror, the error partials,
    // the device copy of the slot table (staged through pinned memory) and the step records
    struct Loop {
        kan::DevBuf ctl;                   // FkLoopCtl [2]
        kan::MappedBuf hmir;               // FkLoopCtl mirror
        kan::DevBuf parts;
        kan::DevBuf dslots;                // [cap]
        kan::PinnedBuf hslots;             // [cap]
        kan::DevBuf ts;                    // [cap] then dts [cap]
        int64_t synced = 0;
        int64_t cap() const { return (int64_t)(dslots.bytes() / sizeof(void*)); }
    } loop;
    // the device-controlled Fisher-KPP adjoint (adjoint_fk_loop): state, mirror, plans, host staging, tables
    struct AdjLoop {
        kan::DevBuf ctl;                   // AdjLoopCtl
        kan::MappedBuf hmir;               // its mirror
        kan::DevBuf plan;                  // AdjLoopPlan [2]
        kan::PinnedBuf hplan;              // pinned staging: a plan and a state
        kan::DevBuf arrive;
        kan::DevBuf meta;
    } aloop;
    kan::DevBuf adj;                 // adjoint scratch (sized on first use)
    // device step control (graph mode): U, K_1..K_7, U_new; control blocks; saveat staging;
    // the dense-output slot table and step times as the device writes them; the cached graph
    struct Graph {
        kan::DevBuf bufs;
        kan::DevBuf ctl;                   // SolveCtl [2], parity-buffered
        kan::PinnedBuf hctl;               // pinned mirror
        kan::DevBuf saveat;
        kan::DevBuf save;
        kan::DevBuf slots;                 // device copy of the slot pointers [cap]
        kan::DevBuf ts, dts;               // [cap] each
        int64_t cap() const { return (int64_t)(ts.bytes() / sizeof(double)); }
        int64_t slots_synced = 0;
        hipStream_t cap_stream = nullptr;
        hipGraphExec_t exec = nullptr;
        // what the graph baked in
        const void* key_p = nullptr;
        int64_t key_nsave = -1, key_cap = -1;
        int key_record = -1, key_steps = -1;
        double key_tf = 0;
        kanode_solver_options key_opt{};
        void drop_exec() {   // a baked-in buffer moved
            if (exec) (void)hipGraphExecDestroy(exec);
            exec = nullptr;
        }
    } g;

    // what is not a buffer: the owned slots, the upload event (with its pending wait), the graph and its stream
    ~kanode_solution() {
        free_slots();
        if (fused.hup_ev) {
            if (fused.hup_pending) (void)hipEventSynchronize(fused.hup_ev);
            (void)hipEventDestroy(fused.hup_ev);
        }
        g.drop_exec();
        if (g.cap_stream) (void)hipStreamDestroy(g.cap_stream);
    }
    // the dense-output slots: one allocation per step, or borrowed views into fused.block
    void free_slots() {
        if (!slots_borrowed)
            for (void* q : slots) (void)hipFree(q);
        slots.clear();
        slots_borrowed = false;
    }
    size_t state_bytes() const { return (size_t)n * esize; }
    char* slot(int64_t i) const { return (char*)slots[record ? i : (i & 1)]; }
    void* u(int64_t i) const { return slot(i); }
    // stage vector k_j (j = 1..7) of step i
    void* k(int64_t i, int j) const {
        if (j == 1) return i == 0 ? k1_0() : k(i - 1, 7);
        if (qform && j == 7) return slot(i) + 5 * state_bytes();
        return slot(i) + (size_t)(j - 1) * state_bytes();
    }
    // the accepted step that holds time t, and θ = (t - t_i) / dt_i in [0, 1] there
    int64_t locate(double t, double& theta) const {
        int64_t i = (int64_t)(std::upper_bound(ts.begin(), ts.end(), t) - ts.begin()) - 1;
        i = std::max<int64_t>(0, std::min<int64_t>((int64_t)ts.size() - 1, i));
        theta = std::min(1.0, std::max(0.0, (t - ts[i]) / dts[i]));
        return i;
    }
    // interpolation polynomial Q_m (m = 1..4) of step i (qform): u(t_i + θ dt_i) = u_i + Σ_m θ^m Q_m
    void* q(int64_t i, int m) const { return slot(i) + (size_t)m * state_bytes(); }
};

#define SOLVE_HIP(h, expr)                                                                                    \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess)                                                                                 \
            return kanode_internal_fail((h), KANODE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define SOLVE_TRY(expr)                            \
    do {                                           \
        kanode_status s_ = (expr);                 \
        if (s_ != KANODE_OK) return s_;            \
    } while (0)

inline bool capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive;
}

// Σ over n entries of ((Σ_j ec_j k_j + ec_last·du) / (abstol + reltol·max(|u|,|y|)))² -> dst (device)
template <typename T>
kanode_status wsumsq(kanode_handle* h, const void* u, const void* y, int nk, const void* const* k, const double* ec,
                     const void* du, double abstol, double reltol, int64_t n, double* dst, hipStream_t st) {
    kan::StageArgs<T> sa{};
    sa.nk = nk;
    for (int j = 0; j < nk; ++j) sa.k[j] = (const T*)k[j];
    for (int j = 0; j <= nk; ++j) sa.ec[j] = ec[j];
    sa.abstol = abstol;
    sa.reltol = reltol;
    SOLVE_HIP(h, kan::launch_stage_error<T>((const T*)u, (const T*)y, (const T*)du, sa, kanode_internal_scratch(h),
                                            kanode_internal_scratch_rows(h), dst, n, st));
    return KANODE_OK;
}

// y = u + Σ_j c_j k_j over n entries (y may alias u)
template <typename T>
kanode_status lincomb(kanode_handle* h, const void* u, int nk, const void* const* k, const double* c, void* y,
                      int64_t n, hipStream_t st) {
    kan::StageArgs<T> sa{};
    sa.nk = nk;
    for (int j = 0; j < nk; ++j) {
        sa.k[j] = (const T*)k[j];
        sa.c[j] = c[j];
    }
    SOLVE_HIP(h, kan::launch_stage_lincomb<T>((const T*)u, sa, (T*)y, n, st));
    return KANODE_OK;
}

inline kanode_status read_scalars(kanode_handle* h, kanode_solution* s, int cnt, hipStream_t st) {
    if (capturing(st)) return kanode_internal_fail(h, KANODE_ERR_CAPTURE, "adaptive step control reads the error norm");
    SOLVE_HIP(h, hipMemcpyAsync(s->hscal(), s->dscal(), cnt * sizeof(double), hipMemcpyDeviceToHost, st));
    SOLVE_HIP(h, hipStreamSynchronize(st));
    return KANODE_OK;
}

// Step-control scalars of the host-controlled adaptive loops: where the producing kernels write them
// (ctl) and how the host gets slots [off, off + cnt) into hscal (read_ctl).
inline double* ctl(kanode_solution* s) { return s->mscal() ? s->mscal() : s->dscal(); }
inline kanode_status read_ctl(kanode_handle* h, kanode_solution* s, int off, int cnt, hipStream_t st) {
    if (capturing(st)) return kanode_internal_fail(h, KANODE_ERR_CAPTURE, "adaptive step control reads the error norm");
    if (!s->mscal())
        SOLVE_HIP(h, hipMemcpyAsync(s->hscal() + off, s->dscal() + off, cnt * sizeof(double), hipMemcpyDeviceToHost, st));
    SOLVE_HIP(h, hipStreamSynchronize(st));
    return KANODE_OK;
}

// Mapped step control without a stream synchronisation: the host marks the slots a step's kernels will
// write with a NaN bit pattern no kernel produces (arm_ctl), launches, and spins until every slot has been
// written (wait_ctl).  A GPU store to coherent host memory is visible to the host within about a
// microsecond, while hipStreamSynchronize's wake-up put ~20 us between the kernel's end and the host's
// next launch (the FK adaptive epoch's kernel trace: a 24 us gap before every step kernel).  The stream
// is queried every few hundred polls: when it has drained, every slot must have been written (kernel
// completion releases the stores), otherwise the call fails instead of spinning forever.
constexpr uint64_t kCtlUnset = 0x7FF4DEADBEEF0001ull;   // a signalling-NaN payload
inline void arm_ctl(double* p, int n) {
    for (int i = 0; i < n; ++i) __atomic_store_n(reinterpret_cast<uint64_t*>(p + i), kCtlUnset, __ATOMIC_RELAXED);
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
}
inline bool ctl_ready(const double* p, int n) {
    for (int i = 0; i < n; ++i)
        if (__atomic_load_n(reinterpret_cast<const uint64_t*>(p + i), __ATOMIC_ACQUIRE) == kCtlUnset) return false;
    return true;
}
struct CtlRange {
    const double* p;
    int n;
};
// spin-wait hint for the host polls of mapped control words
inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield" ::: "memory");
#else
    std::atomic_signal_fence(std::memory_order_seq_cst);
#endif
}
// Spin until done(), a predicate on mapped host memory that the device writes.  The stream is queried every few
// hundred polls: once it has drained every store has landed, so a predicate still false fails with `what`.
template <class Done>
kanode_status spin_until(kanode_handle* h, hipStream_t st, Done done, const char* what) {
    for (uint64_t it = 1; !done(); ++it) {
        if ((it & 255) == 0) {
            const hipError_t q = hipStreamQuery(st);
            if (q == hipSuccess) return done() ? KANODE_OK : kanode_internal_fail(h, KANODE_ERR_HIP, what);
            if (q != hipErrorNotReady) SOLVE_HIP(h, q);
        }
        cpu_relax();
    }
    return KANODE_OK;
}
inline kanode_status wait_ctl(kanode_handle* h, hipStream_t st, std::initializer_list<CtlRange> rs) {
    if (capturing(st)) return kanode_internal_fail(h, KANODE_ERR_CAPTURE, "adaptive step control reads the error norm");
    auto ready = [&] {
        for (const CtlRange& r : rs)
            if (!ctl_ready(r.p, r.n)) return false;
        return true;
    };
    return spin_until(h, st, ready, "step control: the stream drained without the error terms");
}

// Before a solve / adjoint on a solution whose previous call failed: wait for that call's kernels (they may
// still write the mapped slots), then arm every partials slot again, so a polled step control never reads
// an earlier call's values.  The happy path costs nothing.
inline kanode_status ctl_begin(kanode_handle* h, kanode_solution* s, hipStream_t st) {
    if (!s->ctl_dirty) return KANODE_OK;
    if (!capturing(st)) SOLVE_HIP(h, hipStreamSynchronize(st));
    s->fused.saveat_last.clear();   // (an upload of the failed call may not have run)
    s->fused.meta_last.clear();
    if (s->hparts()) arm_ctl(s->hparts(), kanode_internal_max_parts());
    if (s->hscal()) arm_ctl(s->hscal(), kScalars);
    s->ctl_dirty = false;
    return KANODE_OK;
}

inline kanode_stage make_stage(int nk, void* const* k, const double* c) {
    kanode_stage sg{};
    sg.n_prev = nk;
    for (int j = 0; j < nk; ++j) {
        sg.k[j] = k[j];
        sg.c[j] = c[j];
    }
    return sg;
}

struct TableHold {   // p is constant for one solve: each table set is built once
    kanode_handle* h;
    explicit TableHold(kanode_handle* hh) : h(hh) { kanode_internal_hold_tables(h, true); }
    ~TableHold() { kanode_internal_hold_tables(h, false); }
};

// ---- what the drivers share: each fragment stated once ----------------------------------------------------
// The controller fields of a kernel's args struct (they are named as kanode_solver_options names them):
// the tolerances and `adaptive` where the struct has them.
template <class A, class = void>
struct has_tols : std::false_type {};
template <class A>
struct has_tols<A, std::void_t<decltype(std::declval<A&>().abstol)>> : std::true_type {};
template <class A, class = void>
struct has_adaptive : std::false_type {};
template <class A>
struct has_adaptive<A, std::void_t<decltype(std::declval<A&>().adaptive)>> : std::true_type {};
template <class A>
void set_step_opts(A& a, const kanode_solver_options& o) {
    if constexpr (has_tols<A>::value) {
        a.abstol = o.abstol;
        a.reltol = o.reltol;
    }
    a.dtmin = o.dtmin;
    a.beta1 = o.beta1;
    a.beta2 = o.beta2;
    a.gamma = o.gamma;
    a.qmin = o.qmin;
    a.qmax = o.qmax;
    a.qoldinit = o.qoldinit;
    a.maxiters = o.maxiters;
    if constexpr (has_adaptive<A>::value) a.adaptive = o.adaptive ? 1 : 0;
}
// ... and the time span and first step of the one-launch solves (the Chain*Args)
template <class A>
void set_span_opts(A& a, double t0, double tf, const kanode_solver_options& o) {
    a.t0 = t0;
    a.tf = tf;
    a.dt = o.dt;
    set_step_opts(a, o);
}

// The host PI controller (OrdinaryDiffEq's PIController with qsteady_min = qsteady_max = 1) after an attempt of
// size dt with error estimate EEst: rejected -> dt is the size to retry with; accepted -> dt is the next step's
// size and qold the controller's new memory.
struct PiStep {
    bool reject;
    double dt, qold;
};
inline PiStep pi_step(double EEst, double dt, double qold, const kanode_solver_options& o) {
    const double q11 = EEst > 0 ? std::pow(EEst, o.beta1) : 0.0;
    if (EEst > 1.0 && dt > o.dtmin) return {true, dt / std::min(1.0 / o.qmin, q11 / o.gamma), qold};
    double q = q11 / std::pow(qold, o.beta2);
    q = std::max(1.0 / o.qmax, std::min(1.0 / o.qmin, q / o.gamma));
    if (1.0 <= q && q <= 1.0) q = 1.0;   // qsteady_min = qsteady_max = 1
    return {false, q > 0 ? dt / q : dt * o.qmax, std::max(EEst, o.qoldinit)};
}

// Hairer & Wanner's initial step from the norms d0 = |u|, d1 = |f| (then d2 = |f(u + dt0 f) - f| / dt0)
inline double hw_dt0(double d0, double d1, double tdist) {
    const double dt0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    return std::min(dt0, tdist);
}
inline double hw_dt1(double dt0, double d1, double d2, double tdist) {
    const double mx = std::max(d1, d2);
    const double dt1 = mx <= 1e-15 ? std::max(1e-6, dt0 * 1e-3) : std::pow(0.01 / mx, 1.0 / 5.0);
    return std::min(std::min(100 * dt0, dt1), tdist);
}

// the saveat values at or before t0 are u0: rows [0, si) of dst
inline kanode_status copy_saveat_at_t0(kanode_handle* h, const double* saveat, int64_t n_save, double t0, const void* u0,
                                       void* dst, size_t sb, hipStream_t st, int64_t& si) {
    for (si = 0; si < n_save && saveat[si] <= t0 + 1e-14 * std::max(1.0, std::fabs(t0)); ++si)
        SOLVE_HIP(h, hipMemcpyAsync((char*)dst + si * sb, u0, sb, hipMemcpyDeviceToDevice, st));
    return KANODE_OK;
}

inline void set_stats(kanode_solve_stats* stats, int64_t naccept, int64_t nreject, int64_t nf) {
    if (stats) *stats = kanode_solve_stats{naccept, nreject, nf};
}
// the counters a one-launch solve / adjoint left (naccept, nreject, nf, status): status 1 fails with `what`
// (the callers take their own fallback statuses first), else the stats are filled
inline kanode_status finish_one_launch(kanode_handle* h, const int64_t res[4], kanode_solve_stats* stats,
                                       const char* what) {
    if (res[3] == 1) return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, what);
    set_stats(stats, res[0], res[1], res[2]);
    return KANODE_OK;
}

// saveat ascends and ends by te (and, where lo is given, starts at or after *lo); 0 when fine, else which failed
enum { kSaveatOk = 0, kSaveatOrder = 1, kSaveatRange = 2 };
inline int check_saveat(const double* sv, int64_t n, double te, const double* lo = nullptr) {
    for (int64_t j = 1; j < n; ++j)
        if (!(sv[j] >= sv[j - 1])) return kSaveatOrder;
    if (n == 0) return kSaveatOk;
    if (lo && !(sv[0] >= *lo - 1e-12 * std::max(1.0, std::fabs(*lo)))) return kSaveatRange;
    // a stop past te would never be reached and its rows of u_save would stay unwritten
    return sv[n - 1] <= te + 1e-12 * std::max(1.0, std::fabs(te)) ? kSaveatOk : kSaveatRange;
}
inline kanode_status check_saveat(kanode_handle* h, const double* saveat, int64_t n_save, double tf) {
    const int c = check_saveat(saveat, n_save, tf);
    if (c == kSaveatOrder) return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, "saveat must ascend");
    if (c == kSaveatRange) return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, "saveat must lie within [t0, tf]");
    return KANODE_OK;
}

// ---- buffers of the drivers ------------------------------------------------------------------------------
// A stream-ordered upload of host bytes through the solution's pinned staging: unlike hipMemcpy from pageable
// memory it does not hold the host until the stream drains.  The staging is rewritten only after the previous
// upload from it has run (its event).
inline kanode_status staged_upload(kanode_handle* h, kanode_solution* s, void* dst, const void* src, size_t bytes,
                            hipStream_t st, std::vector<char>* last = nullptr) {
    auto& f = s->fused;
    if (last && last->size() == bytes && std::memcmp(last->data(), src, bytes) == 0) return KANODE_OK;
    if (!f.hup_ev) SOLVE_HIP(h, hipEventCreateWithFlags(&f.hup_ev, hipEventDisableTiming));
    if (f.hup_pending) {
        SOLVE_HIP(h, hipEventSynchronize(f.hup_ev));
        f.hup_pending = false;
    }
    SOLVE_HIP(h, f.hup.reserve(bytes));
    std::memcpy(f.hup.ptr(), src, bytes);
    SOLVE_HIP(h, hipMemcpyAsync(dst, f.hup.ptr(), bytes, hipMemcpyHostToDevice, st));
    SOLVE_HIP(h, hipEventRecord(f.hup_ev, st));
    f.hup_pending = true;
    if (last) last->assign((const char*)src, (const char*)src + bytes);
    return KANODE_OK;
}

// The one-launch solves' device copy of saveat and their result block (naccept, nreject, nf, status)
inline kanode_status upload_saveat(kanode_handle* h, kanode_solution* s, const double* saveat, int64_t n_save, hipStream_t st) {
    auto& f = s->fused;
    const size_t bytes = (size_t)n_save * sizeof(double);
    if (f.saveat.bytes() < bytes) {
        f.saveat_last.clear();   // (the device copy moves)
        SOLVE_HIP(h, f.saveat.reserve(bytes));
    }
    SOLVE_HIP(h, f.out.reserve(4 * sizeof(int64_t)));
    if (n_save > 0) SOLVE_TRY(staged_upload(h, s, f.saveat.ptr(), saveat, bytes, st, &f.saveat_last));
    return KANODE_OK;
}

// a mapped mirror the kernels write through its device address (no copy path: it has to have one)
inline kanode_status mapped_reserve(kanode_handle* h, kan::MappedBuf& b, size_t bytes) {
    SOLVE_HIP(h, b.reserve(bytes));
    if (!b.dev<void>()) {
        b.reset();
        return kanode_internal_fail(h, KANODE_ERR_HIP, "hipHostGetDevicePointer: no device address for mapped host memory");
    }
    return KANODE_OK;
}
inline kanode_status dev_oom(kanode_handle* h, const char* what) {
    return kanode_internal_fail(h, KANODE_ERR_ALLOC, std::string("device control: out of device memory (") + what + ")");
}
inline kanode_status dev_reserve(kanode_handle* h, kan::DevBuf& b, size_t bytes, const char* what) {
    return b.reserve(bytes) == hipSuccess ? KANODE_OK : dev_oom(h, what);
}

inline kanode_status check_opts(kanode_handle* h, const kanode_solver_options& o) {
    if (!(o.abstol >= 0) || !(o.reltol >= 0) || o.maxiters < 1 || !(o.qmin > 0) || !(o.qmax > 0) || !(o.gamma > 0))
        return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, "solver options out of range");
    if (!o.adaptive && !(o.dt > 0)) return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, "fixed-step Tsit5 needs dt > 0");
    if (o.control < 0 || o.control > 2 || o.graph_steps < 0)
        return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, "control must be 0 (auto), 1 (host) or 2 (device)");
    return KANODE_OK;
}

// The solution object in *slot for a state of n entries (reused when its shape matches, else made anew): its
// k1_0, control scalars (mapped pinned where the platform allows) and error-partials staging.
inline kanode_status acquire_solution(kanode_handle* h, kanode_solution** slot, int64_t n, int dtype, bool record,
                               hipStream_t st, kanode_solution*& s) {
    s = *slot;
    if (s && (s->h != h || s->n != n || s->dtype != dtype || s->record != record)) {
        // storage of another shape: start over
        if (capturing(st)) return kanode_internal_fail(h, KANODE_ERR_CAPTURE, "dense output of another shape");
        SOLVE_HIP(h, hipStreamSynchronize(st));
        delete s;
        s = nullptr;
        *slot = nullptr;
    }
    if (!s) {
        if (capturing(st)) return kanode_internal_fail(h, KANODE_ERR_CAPTURE, "solve allocates its dense output");
        s = new (std::nothrow) kanode_solution();
        if (!s) return kanode_internal_fail(h, KANODE_ERR_ALLOC, "solution");
        s->h = h;
        s->dtype = dtype;
        s->esize = dtype == KANODE_F64 ? 8 : 4;
        s->n = n;
        s->record = record;
        // (hscal without a device address: the copy path, read_ctl)
        if (s->k1_0_buf.reserve(s->state_bytes()) != hipSuccess || s->dscal_buf.reserve(kScalars * sizeof(double)) != hipSuccess ||
            s->hscal_buf.reserve(kScalars * sizeof(double)) != hipSuccess) {
            delete s;
            return kanode_internal_fail(h, KANODE_ERR_ALLOC, "solve: out of device memory");
        }
        // the partials staging only with its device address; without it the final-reduction launch sums them
        const size_t pb = (size_t)kanode_internal_max_parts() * sizeof(double);
        if (s->mscal() && s->hparts_buf.reserve(pb) == hipSuccess && !s->mparts()) s->hparts_buf.reset();
        if (s->hparts()) arm_ctl(s->hparts(), kanode_internal_max_parts());
    }
    *slot = s;
    return KANODE_OK;
}

// the jump groups and stops of an adjoint over saveat (kanode_adjoint.cpp; the training loop uploads them too)
void adjoint_jump_groups(double t0, double tf, const std::vector<double>& saveat, bool have_dl,
                         std::vector<double>& stops, std::vector<int32_t>& rows, std::vector<int32_t>& off);
