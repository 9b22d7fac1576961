// kanode_solve.cpp — the Tsit5 integrator around the HIP RHS (include/kanode.h: kanode_solve_tsit5);
// its InterpolatingAdjoint is kanode_adjoint.cpp, what both share kanode_solve_internal.hpp.
//
// A native host loop: every Runge-Kutta stage is one kanode_rhs_stage (the stage
// combination u + dt·Σ a_sj k_j is formed inside the RHS kernel, the last stage also
// writes u_new and the embedded-error sum of squares), every adjoint stage one
// kanode_vjp_stage.  The only device->host traffic is the 8-byte error norm of an
// adaptive step (the accept/reject decision); a fixed-step solve never synchronises.
// The step sequence, controller and saveat handling restate OrdinaryDiffEqTsit5 1.1.0 /
// OrdinaryDiffEq 6.89 and SciMLSensitivity 7.69 (third-party, pinned in
// Lotka-Volterra/Manifest.toml; the Python driver kanode/ode.py + kanode/adjoint.py is
// the same algorithm statement and the parity reference of the tests).
#include "kanode_solve_internal.hpp"

extern "C" void kanode_solver_options_default(kanode_solver_options* o) {
    if (!o) return;
    o->abstol = 1e-6;
    o->reltol = 1e-3;
    o->dt = 0.0;
    o->adaptive = 1;
    o->maxiters = 100000;
    o->dtmin = 0.0;
    o->beta1 = 7.0 / 50.0;
    o->beta2 = 2.0 / 25.0;
    o->gamma = 0.9;
    o->qmin = 0.2;
    o->qmax = 10.0;
    o->qoldinit = 1e-4;
    o->control = 0;
    o->graph_steps = 16;
}

extern "C" void kanode_solution_free(kanode_solution* s) { delete s; }
extern "C" int64_t kanode_solution_steps(const kanode_solution* s) { return s ? (int64_t)s->ts.size() : -1; }
extern "C" int64_t kanode_solution_step_sizes(const kanode_solution* s, double* ts, double* dts, int64_t cap) {
    if (!s) return -1;
    const int64_t n = (int64_t)s->ts.size(), m = std::max<int64_t>(0, std::min(n, cap));
    if (ts && m) std::memcpy(ts, s->ts.data(), (size_t)m * sizeof(double));
    if (dts && m) std::memcpy(dts, s->dts.data(), (size_t)m * sizeof(double));
    return n;
}

namespace {

// slots [0, need) exist (allocating — not allowed during capture)
kanode_status ensure_slots(kanode_handle* h, kanode_solution* s, int64_t need, hipStream_t st) {
    if (s->slots_borrowed) s->free_slots();   // the previous solve used the fused block: start a slot list of our own
    if (!s->record) need = std::min<int64_t>(need, 2);
    if ((int64_t)s->slots.size() >= need) return KANODE_OK;
    if (capturing(st)) return kanode_internal_fail(h, KANODE_ERR_CAPTURE, "dense-output storage grows during capture");
    while ((int64_t)s->slots.size() < need) {
        void* p = nullptr;
        if (hipMalloc(&p, 7 * s->state_bytes()) != hipSuccess) {
            (void)hipGetLastError();
            return kanode_internal_fail(h, KANODE_ERR_ALLOC, "dense output: out of device memory at step " +
                                                                 std::to_string(s->slots.size()));
        }
        s->slots.push_back(p);
    }
    return KANODE_OK;
}

// Hairer & Wanner initial step (OrdinaryDiffEq ode_determine_initdt, order 5); kanode/ode.py _initdt
template <typename T>
kanode_status initdt(kanode_handle* h, kanode_solution* s, const void* p, const void* u0, const void* f0,
                     double tdist, const kanode_solver_options& o, double& dt, hipStream_t st, void* tmp) {
    const double one = 1.0;
    double e1[2] = {1.0, 0.0};
    SOLVE_TRY(wsumsq<T>(h, u0, u0, 0, nullptr, &one, u0, o.abstol, o.reltol, s->n, s->dscal() + 0, st));
    SOLVE_TRY(wsumsq<T>(h, u0, u0, 0, nullptr, &one, f0, o.abstol, o.reltol, s->n, s->dscal() + 1, st));
    SOLVE_TRY(read_scalars(h, s, 2, st));
    const double d0 = std::sqrt(s->hscal()[0] / (double)s->n), d1 = std::sqrt(s->hscal()[1] / (double)s->n);
    const double dt0 = hw_dt0(d0, d1, tdist);
    void* kk[1] = {(void*)f0};
    kanode_stage sg = make_stage(1, kk, &dt0);
    SOLVE_TRY(kanode_rhs_stage(h, p, u0, &sg, tmp, s->batch, st));
    const void* kd[1] = {tmp};
    e1[1] = -1.0;
    SOLVE_TRY(wsumsq<T>(h, u0, u0, 1, kd, e1, f0, o.abstol, o.reltol, s->n, s->dscal() + 2, st));
    SOLVE_TRY(read_scalars(h, s, 3, st));
    const double d2 = std::sqrt(s->hscal()[2] / (double)s->n) / dt0;
    dt = hw_dt1(dt0, d1, d2, tdist);
    return KANODE_OK;
}

// The saveat values inside step `step` (t, t + dt] from its dense output: one launch for all of them (the same
// arithmetic as one stage_lincomb / copy each; kan::SaveatStep).  ks: the step's k_1..k_7 (K form).
template <typename T>
kanode_status saveat_in_step(kanode_handle* h, kanode_solution* s, int64_t step, double t, double dt,
                             void* const* ks, const double* saveat, int64_t n_save, int64_t& si, void* u_save,
                             hipStream_t st) {
    const size_t sb = s->state_bytes();
    const double tn = t + dt;
    kan::SaveatStep<T> sv{};
    sv.u = (const T*)s->u(step);
    sv.u_new = (const T*)s->u(step + 1);
    sv.nk = s->qform ? 4 : 7;
    for (int j = 0; j < sv.nk; ++j) sv.k[j] = (const T*)(s->qform ? s->q(step, j + 1) : ks[j]);
    auto flush_sv = [&]() -> kanode_status {
        if (sv.nsv == 0) return KANODE_OK;
        SOLVE_HIP(h, kan::launch_saveat_step<T>(sv, s->n, st));
        sv.nsv = 0;
        sv.exact = 0;
        return KANODE_OK;
    };
    while (si < n_save && saveat[si] <= tn + 1e-12 * std::max(1.0, std::fabs(tn))) {
        const double tsv = saveat[si];
        if (sv.nsv == 0) sv.dst = (T*)((char*)u_save + si * sb);
        const int jv = sv.nsv;
        if (std::fabs(tsv - tn) <= 1e-12 * std::max(1.0, std::fabs(tn))) {
            sv.exact |= 1ull << jv;
        } else if (s->qform) {
            const double th = (tsv - t) / dt;
            sv.w[jv][0] = th;
            sv.w[jv][1] = th * th;
            sv.w[jv][2] = th * th * th;
            sv.w[jv][3] = th * th * th * th;
        } else {
            double w[7];
            interp_weights((tsv - t) / dt, w);
            for (int j = 0; j < 7; ++j) sv.w[jv][j] = w[j] * dt;
        }
        ++sv.nsv;
        ++si;
        if (sv.nsv == kan::kSaveatPerLaunch) SOLVE_TRY(flush_sv());
    }
    return flush_sv();
}

template <typename T>
kanode_status solve_t(kanode_handle* h, const void* p, const void* u0, double t0, double tf, const double* saveat,
                      int64_t n_save, void* u_save, const kanode_solver_options& o, kanode_solution* s,
                      kanode_solve_stats* stats, hipStream_t st) {
    const size_t sb = s->state_bytes();
    int64_t si = 0;
    SOLVE_TRY(copy_saveat_at_t0(h, saveat, n_save, t0, u0, u_save, sb, st, si));
    // fixed step: the whole step sequence is known, allocate it up front
    SOLVE_TRY(ensure_slots(h, s, o.adaptive ? 2 : kanode_fixed_step_count(t0, tf, o.dt, o.maxiters) + 1, st));
    // Fisher-KPP table path: one launch per step and the dense output in Q form
    s->qform = kanode_internal_fk_step_ok(h);
    SOLVE_HIP(h, hipMemcpyAsync(s->u(0), u0, sb, hipMemcpyDeviceToDevice, st));
    kanode_stage s0{};
    SOLVE_TRY(kanode_rhs_stage(h, p, s->u(0), &s0, s->k1_0(), s->batch, st));   // k1 = f(u0)
    double dt = o.dt;
    if (o.adaptive && !(o.dt > 0)) SOLVE_TRY(initdt<T>(h, s, p, s->u(0), s->k1_0(), tf - t0, o, dt, st, s->q(0, 1)));
    double qold = o.qoldinit;
    double t = t0;
    int64_t step = 0, naccept = 0, nreject = 0, nf = 0;
    int64_t it = 0;
    for (; it < o.maxiters; ++it) {
        if (kanode_at_end(t, tf)) break;
        dt = std::min(dt, tf - t);
        SOLVE_TRY(ensure_slots(h, s, step + 2, st));
        void* ks[7];
        for (int j = 0; j < 7; ++j) ks[j] = s->k(step, j + 1);
        bool fused_step = false;   // Fisher-KPP table path: the six stages in one launch
        int nparts = 0;            // > 0: the error is that many partials in hparts (not hscal[0])
        if (o.adaptive && s->mscal()) arm_ctl(s->hscal(), 1);
        double a66[36] = {}, e7[7];   // dt·a_ij, dt·btilde_j of the one-launch steps
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j <= i; ++j) a66[6 * i + j] = dt * TA[i][j];
        for (int j = 0; j < 7; ++j) e7[j] = dt * BT[j];
        if (s->qform) {
            double q47[28];
            for (int m = 0; m < 4; ++m)
                for (int i = 0; i < 7; ++i) q47[7 * m + i] = dt * RI[i][m];
            void* kout[6] = {s->q(step, 1), s->q(step, 2), s->q(step, 3), s->q(step, 4), nullptr, s->k(step, 7)};
            SOLVE_TRY(kanode_internal_fk_step(h, p, s->u(step), ks[0], kout, s->u(step + 1), a66,
                                              o.adaptive ? e7 : nullptr, q47, o.abstol, o.reltol,
                                              o.adaptive ? ctl(s) : nullptr, s->batch, st, fused_step,
                                              o.adaptive ? s->mparts() : nullptr, &nparts));
            if (!fused_step) return kanode_internal_fail(h, KANODE_ERR_HIP, "Tsit5: fused step not launched");
        } else {   // a small chain: the six stages per column in one launch
            SOLVE_TRY(kanode_internal_chain_step(h, p, s->u(step), ks[0], ks + 1, s->u(step + 1), a66,
                                                 o.adaptive ? e7 : nullptr, o.abstol, o.reltol,
                                                 o.adaptive ? ctl(s) : nullptr, s->batch, st, fused_step));
        }
        for (int i = 0; i < 6 && !fused_step; ++i) {
            double c[6];
            for (int j = 0; j <= i; ++j) c[j] = dt * TA[i][j];
            kanode_stage sg = make_stage(i + 1, ks, c);
            if (i == 5) {
                sg.y_out = s->u(step + 1);
                if (o.adaptive) {
                    sg.want_error = 1;
                    for (int j = 0; j < 7; ++j) sg.ec[j] = dt * BT[j];
                    sg.abstol = o.abstol;
                    sg.reltol = o.reltol;
                    sg.error_sumsq = ctl(s);
                }
            }
            SOLVE_TRY(kanode_rhs_stage(h, p, s->u(step), &sg, ks[i + 1], s->batch, st));
        }
        nf += 6;
        double dtnew = dt;
        if (o.adaptive) {
            double sumsq;
            if (nparts > 0) {   // the step kernel's per-block partials, summed here in block order
                SOLVE_TRY(wait_ctl(h, st, {{s->hparts(), nparts}}));
                sumsq = 0.0;
                for (int b = 0; b < nparts; ++b) sumsq += s->hparts()[b];
                arm_ctl(s->hparts(), nparts);   // (every slot stays armed between steps)
            } else {
                if (s->mscal()) SOLVE_TRY(wait_ctl(h, st, {{s->hscal(), 1}}));
                else SOLVE_TRY(read_ctl(h, s, 0, 1, st));
                sumsq = s->hscal()[0];
            }
            const PiStep c = pi_step(std::sqrt(sumsq / (double)s->n), dt, qold, o);
            if (c.reject) {
                ++nreject;
                dt = c.dt;
                continue;
            }
            dtnew = c.dt;
            qold = c.qold;
        }
        const double tn = t + dt;
        SOLVE_TRY(saveat_in_step<T>(h, s, step, t, dt, ks, saveat, n_save, si, u_save, st));
        s->ts.push_back(t);
        s->dts.push_back(dt);
        t = tn;
        ++step;
        ++naccept;
        dt = dtnew;
    }
    if (it == o.maxiters && !kanode_at_end(t, tf))
        return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, "Tsit5: maxiters reached");
    set_stats(stats, naccept, nreject, nf + 1);
    return KANODE_OK;
}

// ---- one-workgroup solve of a small chain (kd_chain_tsit5_kernel) ------------------------
// The whole forward solve in one launch for a chain of small layers and <= 16 trajectories (the
// Lotka-Volterra shape).  done = false when the shape is not covered or the dense-output block
// filled up: the caller then runs the host loop (solve_t) from scratch.
template <typename T>
kanode_status solve_fused_t(kanode_handle* h, const void* p, const void* u0, double t0, double tf, const double* saveat,
                            int64_t n_save, void* u_save, const kanode_solver_options& o, kanode_solution* s,
                            kanode_solve_stats* stats, hipStream_t st, bool& done) {
    done = false;
    if (capturing(st) || !kanode_internal_chain_tsit5_ok(h, s->batch)) return KANODE_OK;
    const size_t sb = s->state_bytes();
    auto& f = s->fused;
    if (s->record) {
        int64_t cap = o.adaptive ? std::min<int64_t>(o.maxiters, 4096) : kanode_fixed_step_count(t0, tf, o.dt, o.maxiters);
        if (const int c = o.adaptive ? kanode_internal_fused_solve_cap(h) : 0) cap = c;   // KANODE_OPT_FUSED_SOLVE_CAP
        cap = std::max<int64_t>(cap, 1);
        if (f.cap(sb) < cap) {
            if (s->slots_borrowed) s->free_slots();   // (they point into the block)
            // no room for the contiguous block: the host loop allocates per step
            if (f.block.reserve((size_t)cap * 7 * sb) != hipSuccess) return KANODE_OK;
        }
        SOLVE_HIP(h, f.ts.reserve(2 * (size_t)f.cap(sb) * sizeof(double)));
    }
    SOLVE_TRY(upload_saveat(h, s, saveat, n_save, st));
    const int64_t fcap = f.cap(sb);
    kan::ChainSolveArgs a{};
    set_span_opts(a, t0, tf, o);
    a.n_save = n_save;
    a.cap = s->record ? fcap : 0;
    a.saveat = f.saveat.as<double>();
    a.u_save = n_save > 0 ? u_save : nullptr;
    a.rec = s->record ? f.block.ptr() : nullptr;
    a.k1_0 = s->k1_0();
    a.ts = s->record ? f.ts.as<double>() : nullptr;
    a.dts = s->record ? f.dts(sb) : nullptr;
    // the counters straight into the mapped host mirror when there is one (no copy launch to read them); without
    // step records to fetch, the host then spins on them instead of synchronising the stream (wait_ctl: the
    // wake-up of hipStreamSynchronize is ~20 us; what follows on the stream is ordered after the kernel anyway)
    // the step records: pinned, mapped host staging the kernel writes alongside the device copy (else copied)
    if (s->record) SOLVE_HIP(h, f.hts.reserve(2 * (size_t)fcap * sizeof(double)));
    double* const hts = f.hts.as<double>();
    a.out = s->mscal() ? (int64_t*)s->mscal() : f.out.as<int64_t>();
    a.hts = s->record && s->mscal() ? f.hts.dev<double>() : nullptr;
    const bool spin = s->mscal() && (!s->record || a.hts);
    if (spin) arm_ctl(s->hscal(), 4);
    bool launched = false;
    SOLVE_TRY(kanode_internal_chain_tsit5(h, p, u0, s->batch, &a, st, launched));
    if (!launched) return KANODE_OK;
    if (!s->mscal()) SOLVE_HIP(h, hipMemcpyAsync(s->hscal(), f.out.ptr(), 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (s->record && !a.hts)
        SOLVE_HIP(h, hipMemcpyAsync(hts, f.ts.ptr(), 2 * (size_t)fcap * sizeof(double), hipMemcpyDeviceToHost, st));
    if (spin) SOLVE_TRY(wait_ctl(h, st, {{s->hscal(), 4}}));
    else SOLVE_HIP(h, hipStreamSynchronize(st));
    int64_t res[4];
    std::memcpy(res, s->hscal(), sizeof(res));
    if (res[3] == 2) return KANODE_OK;   // dense output full: the host loop redoes the solve
    SOLVE_TRY(finish_one_launch(h, res, stats, "Tsit5: maxiters reached"));
    if (s->record) {
        const int64_t na = res[0];
        s->ts.assign(hts, hts + na);
        s->dts.assign(hts + fcap, hts + fcap + na);
        s->free_slots();
        s->slots.resize(fcap);
        for (int64_t i = 0; i < fcap; ++i) s->slots[i] = f.block.as<char>() + (size_t)i * 7 * sb;
        s->slots_borrowed = true;
    }
    done = true;
    return KANODE_OK;
}

// ---- device step control: the solve as a replayed hipGraph ------------------------------
bool same_opts(const kanode_solver_options& a, const kanode_solver_options& b) {
    return a.abstol == b.abstol && a.reltol == b.reltol && a.adaptive == b.adaptive && a.maxiters == b.maxiters &&
           a.dtmin == b.dtmin && a.beta1 == b.beta1 && a.beta2 == b.beta2 && a.gamma == b.gamma && a.qmin == b.qmin &&
           a.qmax == b.qmax && a.qoldinit == b.qoldinit;
}

template <typename T>
kan::Tsit5Bufs<T> graph_bufs(kanode_solution* s) {
    kan::Tsit5Bufs<T> bf{};
    char* b = s->g.bufs.as<char>();
    const size_t sb = s->state_bytes();
    bf.U = (T*)b;
    for (int j = 0; j < 7; ++j) bf.K[j] = (T*)(b + (1 + j) * sb);
    bf.UNEW = (const T*)(b + 8 * sb);
    bf.save = s->g.save.as<T>();
    bf.slots = s->g.slots.as<void*>();
    return bf;
}

// Capture `steps` step slots (six stage launches + tsit5_post_kernel each) into a graph.
template <typename T>
kanode_status build_graph(kanode_handle* h, kanode_solution* s, const void* p, double tf, int64_t n_save,
                          const kanode_solver_options& o, int steps) {
    auto& g = s->g;
    g.drop_exec();
    if (!g.cap_stream) SOLVE_HIP(h, hipStreamCreateWithFlags(&g.cap_stream, hipStreamNonBlocking));
    const kan::Tsit5Bufs<T> bf = graph_bufs<T>(s);
    kan::Tsit5PostArgs pa{};
    pa.tf = tf;
    set_step_opts(pa, o);
    pa.record = s->record;
    pa.n_save = n_save;
    pa.slot_cap = g.cap();
    pa.saveat = g.saveat.as<double>();
    pa.ts_rec = g.ts.as<double>();
    pa.dts_rec = g.dts.as<double>();
    kanode_internal_hold_tables(h, true);   // the first captured stage rebuilds the tables on every replay
    SOLVE_HIP(h, hipStreamBeginCapture(g.cap_stream, hipStreamCaptureModeRelaxed));
    kanode_status r = KANODE_OK;
    for (int sl = 0; sl < steps && r == KANODE_OK; ++sl) {
        kan::SolveCtl* cin = g.ctl.as<kan::SolveCtl>() + (sl & 1);
        kan::SolveCtl* cout = g.ctl.as<kan::SolveCtl>() + ((sl + 1) & 1);
        void* ks[7];
        for (int j = 0; j < 7; ++j) ks[j] = bf.K[j];
        for (int i = 0; i < 6 && r == KANODE_OK; ++i) {
            kanode_stage sg = make_stage(i + 1, ks, TA[i]);
            if (i == 5) {
                sg.y_out = (void*)bf.UNEW;
                if (o.adaptive) {
                    sg.want_error = 1;
                    for (int j = 0; j < 7; ++j) sg.ec[j] = BT[j];
                    sg.abstol = o.abstol;
                    sg.reltol = o.reltol;
                    sg.error_sumsq = s->dscal();
                }
            }
            r = kanode_internal_rhs_stage(h, p, bf.U, &sg, ks[i + 1], s->batch, g.cap_stream, &cin->dt, &cin->done);
        }
        if (r == KANODE_OK) {
            const hipError_t e = kan::launch_tsit5_post<T>(cin, cout, s->dscal(), bf, pa, s->n, g.cap_stream);
            if (e != hipSuccess) r = kanode_internal_fail(h, KANODE_ERR_HIP, std::string("tsit5_post: ") + hipGetErrorString(e));
        }
    }
    hipGraph_t graph = nullptr;
    const hipError_t ec = hipStreamEndCapture(g.cap_stream, &graph);
    if (r != KANODE_OK) {
        if (graph) (void)hipGraphDestroy(graph);
        return r;
    }
    if (ec != hipSuccess) return kanode_internal_fail(h, KANODE_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ec));
    const hipError_t ei = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess) {
        g.exec = nullptr;
        return kanode_internal_fail(h, KANODE_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ei));
    }
    g.key_p = p;
    g.key_nsave = n_save;
    g.key_cap = g.cap();
    g.key_record = s->record;
    g.key_steps = steps;
    g.key_tf = tf;
    g.key_opt = o;
    return KANODE_OK;
}

// dense-output capacity for `need` accepted steps: slots (host + device pointer table) and the
// device step-time records; growing the tables invalidates the graph
kanode_status graph_capacity(kanode_handle* h, kanode_solution* s, int64_t need, hipStream_t st) {
    auto& g = s->g;
    if (s->record) SOLVE_TRY(ensure_slots(h, s, need, st));
    if (need > g.cap()) {
        const int64_t old = g.cap();
        int64_t cap = std::max<int64_t>(64, old);
        while (cap < need) cap *= 2;
        SOLVE_HIP(h, hipStreamSynchronize(st));
        // the slot table is synced again from the host's list; the step records so far are kept
        static const char* const what[] = {"slot table", "step times", "step sizes"};
        int failed = 0;
        const hipError_t e = kan::grow_keep(
            {cap * sizeof(void*), cap * sizeof(double), cap * sizeof(double)}, &failed,
            [&](kan::DevBuf&, kan::DevBuf& nts, kan::DevBuf& ndts) {
                if (old == 0) return hipSuccess;
                const hipError_t c = hipMemcpy(nts.ptr(), g.ts.ptr(), old * sizeof(double), hipMemcpyDeviceToDevice);
                return c != hipSuccess ? c : hipMemcpy(ndts.ptr(), g.dts.ptr(), old * sizeof(double), hipMemcpyDeviceToDevice);
            },
            g.slots, g.ts, g.dts);
        if (e != hipSuccess && failed < 3) return dev_oom(h, what[failed]);
        SOLVE_HIP(h, e);
        g.slots_synced = 0;
    }
    if (s->record && g.slots_synced < (int64_t)s->slots.size()) {
        const int64_t a = g.slots_synced, b = std::min<int64_t>((int64_t)s->slots.size(), g.cap());
        SOLVE_HIP(h, hipMemcpy(g.slots.as<void*>() + a, s->slots.data() + a, (b - a) * sizeof(void*), hipMemcpyHostToDevice));
        g.slots_synced = b;
    }
    return KANODE_OK;
}

template <typename T>
kanode_status solve_graph_t(kanode_handle* h, const void* p, const void* u0, double t0, double tf,
                            const double* saveat, int64_t n_save, void* u_save, const kanode_solver_options& o,
                            kanode_solution* s, kanode_solve_stats* stats, hipStream_t st) {
    auto& g = s->g;
    const size_t sb = s->state_bytes();
    const int steps = o.graph_steps > 0 ? (o.graph_steps + 1) / 2 * 2 : 16;
    // (the graph bakes in bufs, saveat and save: it goes when one of them moves; kernels in flight may use them)
    if (g.bufs.bytes() < 9 * sb) {
        SOLVE_HIP(h, hipStreamSynchronize(st));
        g.drop_exec();
        SOLVE_TRY(dev_reserve(h, g.bufs, 9 * sb, "stage vectors"));
    }
    SOLVE_TRY(dev_reserve(h, g.ctl, 2 * sizeof(kan::SolveCtl), "control"));
    SOLVE_HIP(h, g.hctl.reserve(sizeof(kan::SolveCtl)));
    const size_t saveat_bytes = std::max<int64_t>(n_save, 1) * sizeof(double), save_bytes = std::max<size_t>((size_t)n_save * sb, 1);
    if (g.saveat.bytes() < saveat_bytes || g.save.bytes() < save_bytes) {
        SOLVE_HIP(h, hipStreamSynchronize(st));
        g.drop_exec();
        g.saveat.reset();
        g.save.reset();
        SOLVE_TRY(dev_reserve(h, g.saveat, saveat_bytes, "saveat"));
        SOLVE_TRY(dev_reserve(h, g.save, save_bytes, "saveat values"));
    }
    SOLVE_TRY(kanode_internal_prepare(h, s->batch, st));
    const kan::Tsit5Bufs<T> bf = graph_bufs<T>(s);
    kan::SolveCtl* const hctl = g.hctl.as<kan::SolveCtl>();
    int64_t si = 0;
    SOLVE_TRY(copy_saveat_at_t0(h, saveat, n_save, t0, u0, g.save.ptr(), sb, st, si));
    if (n_save > 0) SOLVE_HIP(h, hipMemcpyAsync(g.saveat.ptr(), saveat, n_save * sizeof(double), hipMemcpyHostToDevice, st));
    SOLVE_HIP(h, hipMemcpyAsync(bf.U, u0, sb, hipMemcpyDeviceToDevice, st));
    kanode_stage s0{};
    SOLVE_TRY(kanode_rhs_stage(h, p, bf.U, &s0, bf.K[0], s->batch, st));   // k1 = f(u0)
    if (s->record) {
        SOLVE_TRY(ensure_slots(h, s, 1, st));
        SOLVE_HIP(h, hipMemcpyAsync(s->k1_0(), bf.K[0], sb, hipMemcpyDeviceToDevice, st));
    }
    double dt = o.dt;
    if (o.adaptive && !(o.dt > 0)) SOLVE_TRY(initdt<T>(h, s, p, bf.U, bf.K[0], tf - t0, o, dt, st, bf.K[1]));
    kan::SolveCtl c0{};
    c0.t = t0;
    c0.dt = std::min(dt, tf - t0);
    c0.qold = o.qoldinit;
    c0.si = si;
    c0.done = kanode_at_end(t0, tf) ? 1 : 0;
    SOLVE_HIP(h, hipStreamSynchronize(st));   // the pinned control block is rewritten below
    *hctl = c0;
    SOLVE_HIP(h, hipMemcpyAsync(g.ctl.ptr(), hctl, sizeof(c0), hipMemcpyHostToDevice, st));
    int64_t naccept = 0;
    for (;;) {
        SOLVE_TRY(graph_capacity(h, s, naccept + steps + 1, st));
        if (!g.exec || g.key_p != p || g.key_nsave != n_save || g.key_cap != g.cap() || g.key_record != (int)s->record ||
            g.key_steps != steps || g.key_tf != tf || !same_opts(g.key_opt, o))
            SOLVE_TRY(build_graph<T>(h, s, p, tf, n_save, o, steps));
        SOLVE_HIP(h, hipGraphLaunch(g.exec, st));
        SOLVE_HIP(h, hipMemcpyAsync(hctl, g.ctl.ptr(), sizeof(kan::SolveCtl), hipMemcpyDeviceToHost, st));
        SOLVE_HIP(h, hipStreamSynchronize(st));
        naccept = hctl->naccept;
        if (hctl->done) break;
    }
    const kan::SolveCtl c = *hctl;
    if (c.status == 1) return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, "Tsit5: maxiters reached");
    if (c.status != 0) return kanode_internal_fail(h, KANODE_ERR_ALLOC, "Tsit5 (device control): dense-output storage full");
    if (s->record && c.naccept > 0) {
        s->ts.resize(c.naccept);
        s->dts.resize(c.naccept);
        SOLVE_HIP(h, hipMemcpy(s->ts.data(), g.ts.ptr(), c.naccept * sizeof(double), hipMemcpyDeviceToHost));
        SOLVE_HIP(h, hipMemcpy(s->dts.data(), g.dts.ptr(), c.naccept * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (n_save > 0) SOLVE_HIP(h, hipMemcpyAsync(u_save, g.save.ptr(), n_save * sb, hipMemcpyDeviceToDevice, st));
    set_stats(stats, c.naccept, c.nreject, 6 * c.attempts + 1);
    return KANODE_OK;
}

// ---- the adaptive Fisher-KPP solve with the step control on the device ------------------------------
// KANODE_OPT_FK_DEVICE_LOOP, control = auto, fp64 table path, dense output kept: solve_t's algorithm with every
// attempt one launch of the step kernel's DEV instantiation (kan::FkLoopArgs): launch q decides attempt q - 1 at
// its head (every workgroup, the same sums) and takes the next, so the host queues launches ahead in batches of
// kBatch and only polls the mapped mirror of the state; launches queued past the end return at once.  The saveat values come from the dense output afterwards (saveat_in_step, as solve_t).
// done = false when not covered (solve_t runs instead).
kanode_status solve_fk_loop(kanode_handle* h, const void* p, const void* u0, double t0, double tf,
                            const double* saveat, int64_t n_save, void* u_save, const kanode_solver_options& o,
                            kanode_solution* s, kanode_solve_stats* stats, hipStream_t st, bool& done) {
    done = false;
    if (o.control != 0 || !o.adaptive || !s->record || s->dtype != KANODE_F64 || capturing(st) ||
        !kanode_internal_fk_loop_ok(h) || kanode_at_end(t0, tf))
        return KANODE_OK;
    constexpr int64_t kBatch = 16;
    const size_t sb = s->state_bytes();
    auto& L = s->loop;
    // the slot table and step records grow geometrically with the launches queued (a solve that reaches
    // maxiters stops on the device's status 2, not on the table size)
    const int64_t cap_max = o.maxiters + 2 * kBatch + 3;
    auto grow = [&](int64_t want) -> kanode_status {
        const int64_t old = L.cap();
        if (old >= want) return KANODE_OK;
        int64_t cap = std::max<int64_t>(old, 1024);
        while (cap < want) cap *= 2;
        cap = std::max(std::min(cap, cap_max), want);
        SOLVE_HIP(h, hipStreamSynchronize(st));   // (the queued launches write the old records)
        int failed = 0;
        const hipError_t e = kan::grow_keep(
            {cap * sizeof(void*), 2 * cap * sizeof(double), cap * sizeof(void*)}, &failed,
            [&](kan::DevBuf& nslots, kan::DevBuf& nts, kan::PinnedBuf& nh) {
                if (old == 0) return hipSuccess;
                // keep what is recorded: slots [0, synced), ts | dts (each cap long)
                const double* ots = L.ts.as<double>();
                hipError_t c = hipMemcpy(nslots.ptr(), L.dslots.ptr(), old * sizeof(void*), hipMemcpyDeviceToDevice);
                if (c == hipSuccess) c = hipMemcpy(nts.ptr(), ots, old * sizeof(double), hipMemcpyDeviceToDevice);
                if (c == hipSuccess)
                    c = hipMemcpy(nts.as<double>() + cap, ots + old, old * sizeof(double), hipMemcpyDeviceToDevice);
                if (c == hipSuccess) std::memcpy(nh.ptr(), L.hslots.ptr(), old * sizeof(void*));
                return c;
            },
            L.dslots, L.ts, L.hslots);
        if (e != hipSuccess && failed == 0) return dev_oom(h, "slot table");
        if (e != hipSuccess && failed == 1) return dev_oom(h, "step records");
        if (e != hipSuccess && failed == 2)
            return kanode_internal_fail(h, KANODE_ERR_ALLOC, "Tsit5 (device loop): pinned slot staging");
        SOLVE_HIP(h, e);
        return KANODE_OK;
    };
    SOLVE_TRY(grow(std::min<int64_t>(cap_max, 4 * kBatch + 3)));
    SOLVE_TRY(dev_reserve(h, L.ctl, 2 * sizeof(kan::FkLoopCtl), "loop state"));
    SOLVE_TRY(dev_reserve(h, L.parts, 2 * kanode_internal_max_parts() * sizeof(double), "loop partials"));
    SOLVE_TRY(mapped_reserve(h, L.hmir, sizeof(kan::FkLoopCtl)));
    kan::FkLoopCtl* const hmir = L.hmir.as<kan::FkLoopCtl>();
    L.synced = 0;
    int64_t si = 0;
    SOLVE_TRY(copy_saveat_at_t0(h, saveat, n_save, t0, u0, u_save, sb, st, si));
    SOLVE_TRY(ensure_slots(h, s, 3, st));
    s->qform = true;
    SOLVE_HIP(h, hipMemcpyAsync(s->u(0), u0, sb, hipMemcpyDeviceToDevice, st));
    kanode_stage s0{};
    SOLVE_TRY(kanode_rhs_stage(h, p, s->u(0), &s0, s->k1_0(), s->batch, st));   // k1 = f(u0)
    double dt = o.dt;
    if (!(o.dt > 0)) SOLVE_TRY(initdt<double>(h, s, p, s->u(0), s->k1_0(), tf - t0, o, dt, st, s->q(0, 1)));
    SOLVE_HIP(h, hipStreamSynchronize(st));   // (the mirror is the init copy's source and the device's target)
    kan::FkLoopCtl c0{};   // launch 0 reads state[1]: no attempt pending
    c0.t = t0;
    c0.dt = dt;
    c0.qold = o.qoldinit;
    c0.cand[1] = s->slots[0];
    c0.cand[2] = s->slots[1];
    c0.cand[3] = s->slots[2];
    *hmir = c0;
    SOLVE_HIP(h, hipMemcpy(L.ctl.as<kan::FkLoopCtl>() + 1, &c0, sizeof(c0), hipMemcpyHostToDevice));
    kan::FkLoopArgs la{};
    la.state = L.ctl.as<kan::FkLoopCtl>();
    la.mirror = L.hmir.dev<kan::FkLoopCtl>();
    auto set_tables = [&] {   // (again after grow)
        la.slots = L.dslots.as<void*>();
        la.ts = L.ts.as<double>();
        la.dts = la.ts + L.cap();
    };
    set_tables();
    la.k1_0 = (const double*)s->k1_0();
    la.parts = L.parts.as<double>();
    la.max_grid = kanode_internal_max_parts();
    la.n = s->n;
    la.tf = tf;
    set_step_opts(la, o);
    const volatile kan::FkLoopCtl* mir = hmir;
    int64_t queued = 0;
    for (;;) {
        if (queued + kBatch + 3 > L.cap()) {
            if (queued + kBatch + 3 > cap_max)
                return kanode_internal_fail(h, KANODE_ERR_ALLOC, "Tsit5 (device loop): step table full");
            SOLVE_TRY(grow(queued + kBatch + 3));
            set_tables();
        }
        // slots for every step the queued launches can reach (each launch advances at most one step; a state
        // names the slots up to its step + 2)
        SOLVE_TRY(ensure_slots(h, s, queued + kBatch + 3, st));
        const int64_t ns = (int64_t)s->slots.size();
        if (L.synced < ns) {
            void** const hsl = L.hslots.as<void*>();
            std::memcpy(hsl + L.synced, s->slots.data() + L.synced, (ns - L.synced) * sizeof(void*));
            SOLVE_HIP(h, hipMemcpyAsync(L.dslots.as<void*>() + L.synced, hsl + L.synced, (ns - L.synced) * sizeof(void*),
                                        hipMemcpyHostToDevice, st));
            L.synced = ns;
        }
        for (int64_t i = 0; i < kBatch; ++i)
            SOLVE_TRY(kanode_internal_fk_step_loop(h, p, &la, queued + i, s->batch, st));
        queued += kBatch;
        // keep one batch queued behind the running one: wait until the device has decided the previous batch's
        // attempts (launch q decides attempt q - 1)
        SOLVE_TRY(spin_until(h, st, [&] { return mir->status != 0 || mir->it + 1 >= queued - kBatch; },
                             "Tsit5 (device loop): the stream drained without progress"));
        if (mir->status != 0) break;
    }
    SOLVE_HIP(h, hipStreamSynchronize(st));
    const kan::FkLoopCtl c = *hmir;
    if (c.status == 2) return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, "Tsit5: maxiters reached");
    s->ts.resize(c.step);
    s->dts.resize(c.step);
    if (c.step > 0) {
        SOLVE_HIP(h, hipMemcpy(s->ts.data(), la.ts, c.step * sizeof(double), hipMemcpyDeviceToHost));
        SOLVE_HIP(h, hipMemcpy(s->dts.data(), la.dts, c.step * sizeof(double), hipMemcpyDeviceToHost));
    }
    for (int64_t i = 0; i < c.step && si < n_save; ++i)
        SOLVE_TRY(saveat_in_step<double>(h, s, i, s->ts[i], s->dts[i], nullptr, saveat, n_save, si, u_save, st));
    set_stats(stats, c.step, c.nreject, 6 * c.it + 1);
    done = true;
    return KANODE_OK;
}

}  // namespace

extern "C" kanode_status kanode_solve_tsit5(kanode_handle* h, const void* p, const void* u0, int64_t batch, double t0,
                                            double tf, const double* saveat, int64_t n_save, void* u_save,
                                            const kanode_solver_options* opt, kanode_solution** dense,
                                            kanode_solve_stats* stats, void* stream) {
    SOLVE_TRY(kanode_internal_check(h));
    const kanode_solver_options o = resolved(opt);
    SOLVE_TRY(check_opts(h, o));
    if (!p || !u0 || batch < 1 || !(tf > t0) || n_save < 0 || (n_save > 0 && (!saveat || !u_save)))
        return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, "solve: null pointer, batch < 1 or tf <= t0");
    if (!kanode_internal_square(h))
        return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, "solve needs an RHS with N_in == N_out");
    SOLVE_TRY(check_saveat(h, saveat, n_save, tf));
    hipStream_t st = (hipStream_t)stream;
    const int dtype = kanode_internal_dtype(h);
    const int64_t n = kanode_internal_state_length(h) * batch;
    // without a dense output the handle keeps the solve's storage (and any cached graph) for the next call
    const bool record = dense != nullptr;
    kanode_solution** slot = record ? dense : (kanode_solution**)kanode_internal_solution_cache(h);
    kanode_solution* s = nullptr;
    SOLVE_TRY(acquire_solution(h, slot, n, dtype, record, st, s));
    s->batch = batch;
    s->t0 = t0;
    s->tf = tf;
    s->saveat.assign(saveat, saveat + n_save);
    s->ts.clear();
    s->dts.clear();
    s->qform = false;   // K-form dense output unless the host loop takes the Fisher-KPP step path
    kanode_status r = ctl_begin(h, s, st);
    if (r == KANODE_OK) {
        TableHold hold(h);
        // auto = host: a replayed graph node costs the GPU what an eager launch does (ROCm 7.2,
        // tools/solve_modes.py), so device control only wins where the per-step norm read is a
        // large part of a step (adaptive, small states); it is opt-in
        const bool dev = o.control == 2;
        if (dev && capturing(st)) {
            r = kanode_internal_fail(h, KANODE_ERR_CAPTURE, "device step control cannot run inside a capture");
        } else if (dev) {
            r = dtype == KANODE_F64 ? solve_graph_t<double>(h, p, u0, t0, tf, saveat, n_save, u_save, o, s, stats, st)
                                    : solve_graph_t<float>(h, p, u0, t0, tf, saveat, n_save, u_save, o, s, stats, st);
        } else {
            // auto: a small chain (<= 16 trajectories) runs the whole solve in one workgroup
            bool done = false;
            r = KANODE_OK;
            if (o.control == 0)
                r = dtype == KANODE_F64
                        ? solve_fused_t<double>(h, p, u0, t0, tf, saveat, n_save, u_save, o, s, stats, st, done)
                        : solve_fused_t<float>(h, p, u0, t0, tf, saveat, n_save, u_save, o, s, stats, st, done);
            if (r == KANODE_OK && !done)   // auto: the adaptive Fisher-KPP table path with the control on the device
                r = solve_fk_loop(h, p, u0, t0, tf, saveat, n_save, u_save, o, s, stats, st, done);
            if (r == KANODE_OK && !done)
                r = dtype == KANODE_F64 ? solve_t<double>(h, p, u0, t0, tf, saveat, n_save, u_save, o, s, stats, st)
                                        : solve_t<float>(h, p, u0, t0, tf, saveat, n_save, u_save, o, s, stats, st);
        }
    }
    if (r != KANODE_OK) s->ctl_dirty = true;
    if (record || s->state_bytes() <= (size_t)64 << 20) {
        *slot = s;   // kept for the next solve (a large scratch solve gives its memory back)
    } else {
        if (hipStreamSynchronize(st) != hipSuccess) (void)hipGetLastError();
        delete s;
        *slot = nullptr;
    }
    return r;
}
