// kanode_adjoint.cpp — the InterpolatingAdjoint of kanode_solve_tsit5's dense output (include/kanode.h:
// kanode_adjoint_tsit5): the host loop adjoint_t with one kanode_vjp_stage per stage, its device-controlled
// Fisher-KPP form, and the one-launch adjoints of a small chain and of the surrogate pair.
// (SciMLSensitivity 7.69's InterpolatingAdjoint; kanode/adjoint.py is the same algorithm statement.)
#include "kanode_solve_internal.hpp"

namespace {

// KANODE_OPT_RECORD_ADJOINT_STEPS: the device record of a device-controlled adjoint's accepted step sizes
kanode_status adjoint_step_record(kanode_handle* h, kanode_solution* s, double*& hs, int64_t& hs_cap) {
    SOLVE_HIP(h, s->hs_dev.reserve((4 * s->ts.size() + 1024) * sizeof(double)));
    hs = s->hs_dev.as<double>();
    hs_cap = (int64_t)(s->hs_dev.bytes() / sizeof(double));
    return KANODE_OK;
}

// ---- the adaptive Fisher-KPP adjoint with its step control on the device (kan_adjloop.hpp) ----------------
// adjoint_t's loop for the combined adaptive rows step (KANODE_OPT_FK_DEVICE_LOOP): one attempt = the rows
// launch + the finish launch, whose last workgroup runs the controller and plans the next attempt; the host
// queues attempts in batches and only polls the mapped mirror of the state.  A step landing on a saveat stop
// pauses the loop: the host drains the stream, takes the stop (take_stop: the jump and the FSAL
// re-evaluation, as its own loop), plans the next attempt and resumes.  On return the loop's variables hold
// adjoint_t's values at its end.
template <class TakeStop>
kanode_status adjoint_fk_loop(kanode_handle* h, const void* p, kanode_solution* s, const kanode_solver_options& o,
                              const std::vector<double>& stops, double* slab, int64_t grid, void* const* lam,
                              void* const* kl, void* const* mu, void* const* km, double& hstep, double& qold,
                              double& tau, size_t& si, int64_t& naccept, int64_t& nreject, int64_t& it, int64_t& nf,
                              int& lcur, int& mcur, std::vector<double>* hrec, TakeStop& take_stop, hipStream_t st) {
    constexpr int64_t kBatch = 16;
    const int64_t nsteps = (int64_t)s->ts.size(), P = kanode_param_length(h), nst = (int64_t)stops.size();
    auto& A = s->aloop;
    // device copies: forward slot table | ts | dts | stops, then the error terms [1 + P]
    const size_t meta = (size_t)(3 * nsteps + nst + 1 + P + 8) * sizeof(double);
    if (A.meta.bytes() < meta) {
        SOLVE_HIP(h, hipStreamSynchronize(st));
        SOLVE_TRY(dev_reserve(h, A.meta, meta, "adjoint loop tables"));
    }
    SOLVE_TRY(dev_reserve(h, A.ctl, sizeof(kan::AdjLoopCtl), "adjoint loop state"));
    SOLVE_TRY(dev_reserve(h, A.plan, 2 * sizeof(kan::AdjLoopPlan), "adjoint loop plans"));
    SOLVE_TRY(dev_reserve(h, A.arrive, 64, "adjoint loop counter"));
    SOLVE_TRY(mapped_reserve(h, A.hmir, sizeof(kan::AdjLoopCtl)));
    SOLVE_HIP(h, A.hplan.reserve(sizeof(kan::AdjLoopPlan) + sizeof(kan::AdjLoopCtl)));
    kan::AdjLoopCtl* const hmir = A.hmir.as<kan::AdjLoopCtl>();
    kan::AdjLoopPlan* const hp = A.hplan.as<kan::AdjLoopPlan>();   // then the state
    kan::AdjLoopPlan* const dplan = A.plan.as<kan::AdjLoopPlan>();
    void** dslots = A.meta.as<void*>();
    double* dts_ = A.meta.as<double>() + nsteps;   // [ts | dts]
    double* dstops = dts_ + 2 * nsteps;
    double* dout = dstops + nst;
    {
        std::vector<char> host((3 * nsteps + nst) * sizeof(double));
        std::memcpy(host.data(), s->slots.data(), nsteps * sizeof(void*));
        std::memcpy(host.data() + nsteps * sizeof(double), s->ts.data(), nsteps * sizeof(double));
        std::memcpy(host.data() + 2 * nsteps * sizeof(double), s->dts.data(), nsteps * sizeof(double));
        std::memcpy(host.data() + 3 * nsteps * sizeof(double), stops.data(), nst * sizeof(double));
        SOLVE_HIP(h, hipStreamSynchronize(st));
        SOLVE_HIP(h, hipMemcpy(A.meta.ptr(), host.data(), host.size(), hipMemcpyHostToDevice));
    }
    SOLVE_HIP(h, hipMemsetAsync(A.arrive.ptr(), 0, sizeof(unsigned), st));
    kan::AdjLoopArgs la{};
    la.ctl = A.ctl.as<kan::AdjLoopCtl>();
    la.mirror = A.hmir.dev<kan::AdjLoopCtl>();
    la.plan = dplan;
    la.arrive = A.arrive.as<unsigned>();
    for (int i = 0; i < 2; ++i) {
        la.lam[i] = (double*)lam[i];
        la.mu[i] = (double*)mu[i];
    }
    for (int j = 0; j < 7; ++j) {
        la.kl[j] = (double*)kl[j];
        la.km[j] = (double*)km[j];
    }
    la.slots = dslots;
    la.fts = dts_;
    la.fdts = dts_ + nsteps;
    la.nsteps = nsteps;
    la.slab = slab;
    la.grid = grid;
    la.P = P;
    la.n = s->n;
    la.out = dout;
    la.stops = dstops;
    la.nstops = nst;
    la.tf = s->tf;
    la.TT = s->tf - s->t0;
    set_step_opts(la, o);
    la.ntot = (double)(s->n + P);
    if (hrec) SOLVE_TRY(adjoint_step_record(h, s, la.hs, la.hs_cap));
    // the host's view of the forward steps for the plans it builds (the same values as the device's)
    struct HostFw {
        const kanode_solution* s;
        double ts(int64_t i) const { return s->ts[i]; }
        double dts(int64_t i) const { return s->dts[i]; }
        const void* slot(int64_t i) const { return s->u(i); }
    } hfw{s};
    kan::AdjLoopCtl c{};
    c.tau = tau;
    c.h = hstep;
    c.qold = qold;
    c.si = (int64_t)si;
    c.naccept = naccept;
    c.nreject = nreject;
    c.it = it;
    c.nf = nf;
    c.fi = nsteps - 1;
    c.lc = lcur;
    c.mc = mcur;
    c.fs = 0;
    const volatile kan::AdjLoopCtl* mir = hmir;
    for (;;) {
        // (re)start at c: the loop top, the attempt's plan, the state (the stream is drained: the staging is free)
        kan::adj_loop_top(la, c, stops[(size_t)c.si]);   // (la.stops is the device copy)
        if (c.status != 0) break;
        kan::adj_loop_plan(la, c, *hp, hfw);
        std::memcpy(hp + 1, &c, sizeof(c));
        *hmir = c;
        // both buffers: the device rewrites only a plan's step-dependent fields (adj_finish_loop_kernel)
        for (int b = 0; b < 2; ++b)
            SOLVE_HIP(h, hipMemcpyAsync(dplan + b, hp, sizeof(kan::AdjLoopPlan), hipMemcpyHostToDevice, st));
        SOLVE_HIP(h, hipMemcpyAsync(la.ctl, hp + 1, sizeof(c), hipMemcpyHostToDevice, st));
        const int64_t base = c.it;
        int64_t queued = 0;
        for (;;) {
            for (int64_t i = 0; i < kBatch; ++i) SOLVE_TRY(kanode_internal_fk_adjoint_loop(h, p, &la, s->batch, st));
            queued += kBatch;
            SOLVE_TRY(spin_until(h, st, [&] { return mir->status != 0 || mir->it >= base + queued - kBatch; },
                                 "adjoint Tsit5 (device loop): the stream drained without progress"));
            if (mir->status != 0) break;
        }
        SOLVE_HIP(h, hipStreamSynchronize(st));
        c = *hmir;
        if (c.status != 3) break;
        // paused on stops[si]: the stop's jump and FSAL re-evaluation on the host, then the next stop
        tau = c.tau;
        si = (size_t)c.si;
        lcur = c.lc;
        nf = c.nf;
        SOLVE_TRY(take_stop(c.fs ? kl[6] : kl[0], c.fs ? km[6] : km[0]));
        SOLVE_TRY(kanode_internal_vjp_flush(h, st));
        c.lc = lcur;
        c.si = (int64_t)si;
        c.nf = nf;
        c.status = 0;
    }
    if (c.status == 2) {
        it = o.maxiters;   // (adjoint_t reports it)
        tau = c.tau;
        return KANODE_OK;
    }
    tau = c.tau;
    hstep = c.h;
    qold = c.qold;
    si = (size_t)c.si;
    naccept = c.naccept;
    nreject = c.nreject;
    it = c.it;
    nf = c.nf;
    lcur = c.lc;
    mcur = c.mc;
    if (hrec && la.hs) {
        hrec->resize((size_t)std::min(naccept, la.hs_cap));
        if (!hrec->empty())
            SOLVE_HIP(h, hipMemcpy(hrec->data(), la.hs, hrec->size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    return KANODE_OK;
}

// ---- InterpolatingAdjoint -----------------------------------------------------------
template <typename T>
kanode_status adjoint_t(kanode_handle* h, const void* p, kanode_solution* s, const void* dl_du, void* du0, void* dp,
                        const kanode_solver_options& o, kanode_solve_stats* stats, hipStream_t st) {
    const int64_t n = s->n, P = kanode_param_length(h);
    const size_t sb = s->state_bytes(), pb = (size_t)P * s->esize;
    const int64_t nsteps = (int64_t)s->ts.size();
    if (nsteps < 1) return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, "adjoint: the forward solve took no steps");
    // scratch: lam[2], kl[7] (states), mu[2], km[7] (parameter vectors)
    const size_t need = 9 * sb + 9 * pb + 256;
    if (s->adj.bytes() < need) {
        if (capturing(st)) return kanode_internal_fail(h, KANODE_ERR_CAPTURE, "adjoint scratch grows during capture");
        SOLVE_HIP(h, hipStreamSynchronize(st));
        if (s->adj.reserve(need) != hipSuccess)
            return kanode_internal_fail(h, KANODE_ERR_ALLOC, "adjoint scratch: out of device memory");
    }
    auto align = [](size_t x) { return (x + 255) & ~(size_t)255; };
    char* w = s->adj.as<char>();
    void *lam[2], *kl[7], *mu[2], *km[7];
    for (auto& x : lam) { x = w; w += sb; }
    for (auto& x : kl) { x = w; w += sb; }
    w = s->adj.as<char>() + align(9 * sb);
    for (auto& x : mu) { x = w; w += pb; }
    for (auto& x : km) { x = w; w += pb; }

    const double t0 = s->t0, tf = s->tf, TT = tf - t0;
    const double eps = 1e-12 * std::max(1.0, std::fabs(tf));
    // jumps: distinct saveat values, each with the rows of dl_du that land on it
    struct Jump { double ts; std::vector<int64_t> rows; bool live; };
    std::vector<Jump> jumps;
    for (int64_t j = 0; j < (int64_t)s->saveat.size(); ++j) {
        auto f = std::find_if(jumps.begin(), jumps.end(), [&](const Jump& x) { return x.ts == s->saveat[j]; });
        if (f == jumps.end()) jumps.push_back({s->saveat[j], {j}, true});
        else f->rows.push_back(j);
    }
    auto add_jump = [&](Jump& jm, void* l) -> kanode_status {
        for (int64_t r : jm.rows) {
            const void* g[1] = {(const char*)dl_du + r * sb};
            const double one = 1.0;
            SOLVE_TRY(lincomb<T>(h, l, 1, g, &one, l, n, st));
        }
        jm.live = false;
        return KANODE_OK;
    };
    SOLVE_HIP(h, hipMemsetAsync(lam[0], 0, sb, st));
    SOLVE_HIP(h, hipMemsetAsync(mu[0], 0, pb, st));
    if (dl_du) {
        for (auto& jm : jumps)
            if (jm.live && jm.ts == tf) SOLVE_TRY(add_jump(jm, lam[0]));
    } else {
        for (auto& jm : jumps) jm.live = false;
    }
    std::vector<double> stops;
    for (auto& jm : jumps)
        if (jm.live && t0 + eps < jm.ts && jm.ts < tf - eps) stops.push_back(tf - jm.ts);
    std::sort(stops.begin(), stops.end());
    stops.push_back(TT);

    // adjoint RHS at τ: u(tf - τ) from the dense output, λ stage input l + Σ lc_j lks_j
    // (-> lam_out), lamJ = λsᵀ∂f/∂u, dpo = λsᵀ∂f/∂p; ec != NULL adds the λ error total -> err
    // defer: the dp / error reductions of this stage wait for flush() (one launch per step)
    kanode_internal_vjp_discard(h);   // nothing pending from an earlier failed call
    int lam_parts = 0;                // > 0: the step's λ error as that many partials in hparts
    struct PartsOff {                 // the handle must not keep the solution's buffer past this call
        kanode_handle* h;
        ~PartsOff() { kanode_internal_set_err_parts(h, nullptr, nullptr); }
    } parts_off{h};
    if (o.adaptive && s->mparts()) kanode_internal_set_err_parts(h, s->mparts(), &lam_parts);
    auto adj_rhs = [&](double tau, const void* l, int nl, void* const* lks, const double* lc, void* lamJ, void* dpo,
                       void* lam_out, const double* ec, double* err, bool defer = false) -> kanode_status {
        const double t = tf - tau;
        double theta;
        const int64_t i = s->locate(t, theta);
        const double dti = s->dts[i];
        kanode_stage su;
        if (s->qform) {   // u_i + Σ_m θ^m Q_m
            const double c[4] = {theta, theta * theta, theta * theta * theta, theta * theta * theta * theta};
            void* qs[4] = {s->q(i, 1), s->q(i, 2), s->q(i, 3), s->q(i, 4)};
            su = make_stage(4, qs, c);
        } else {
            double c[7];
            interp_weights(theta, c);
            for (double& x : c) x *= dti;
            void* ks[7];
            for (int j = 0; j < 7; ++j) ks[j] = s->k(i, j + 1);
            su = make_stage(7, ks, c);
        }
        kanode_stage sl = make_stage(nl, lks, lc);
        sl.y_out = lam_out;
        if (ec) {
            sl.want_error = 1;
            for (int j = 0; j <= nl; ++j) sl.ec[j] = ec[j];
            sl.abstol = o.abstol;
            sl.reltol = o.reltol;
            sl.error_sumsq = err;
        }
        return kanode_internal_vjp_stage(h, p, s->u(i), &su, l, &sl, lamJ, dpo, true, s->batch, st, nullptr, nullptr,
                                         defer);
    };
    const int64_t ntot = n + P;
    int lcur = 0, mcur = 0;   // lam[lcur], mu[mcur] hold λ, μ (a saveat jump flips λ alone)
    SOLVE_TRY(adj_rhs(0.0, lam[lcur], 0, nullptr, nullptr, kl[0], km[0], nullptr, nullptr, nullptr));
    int64_t nf = 1;
    double hstep = o.dt;
    if (o.adaptive && !(o.dt > 0)) {
        // Hairer-Wanner on the augmented state [λ; μ] (kanode/adjoint.py)
        const double one = 1.0;
        SOLVE_TRY(wsumsq<T>(h, lam[lcur], lam[lcur], 0, nullptr, &one, lam[lcur], o.abstol, o.reltol, n, s->dscal() + 0, st));
        SOLVE_TRY(wsumsq<T>(h, mu[mcur], mu[mcur], 0, nullptr, &one, mu[mcur], o.abstol, o.reltol, P, s->dscal() + 1, st));
        SOLVE_TRY(wsumsq<T>(h, lam[lcur], lam[lcur], 0, nullptr, &one, kl[0], o.abstol, o.reltol, n, s->dscal() + 2, st));
        SOLVE_TRY(wsumsq<T>(h, mu[mcur], mu[mcur], 0, nullptr, &one, km[0], o.abstol, o.reltol, P, s->dscal() + 3, st));
        SOLVE_TRY(read_scalars(h, s, 4, st));
        const double d0 = std::sqrt((s->hscal()[0] + s->hscal()[1]) / (double)ntot);
        const double d1 = std::sqrt((s->hscal()[2] + s->hscal()[3]) / (double)ntot);
        const double h0 = hw_dt0(d0, d1, TT);
        void* k1l[1] = {kl[0]};
        SOLVE_TRY(adj_rhs(h0, lam[lcur], 1, k1l, &h0, kl[1], km[1], nullptr, nullptr, nullptr));
        ++nf;
        const double e2[2] = {1.0, -1.0};
        const void* a1[1] = {kl[1]};
        const void* b1[1] = {km[1]};
        SOLVE_TRY(wsumsq<T>(h, lam[lcur], lam[lcur], 1, a1, e2, kl[0], o.abstol, o.reltol, n, s->dscal() + 0, st));
        SOLVE_TRY(wsumsq<T>(h, mu[mcur], mu[mcur], 1, b1, e2, km[0], o.abstol, o.reltol, P, s->dscal() + 1, st));
        SOLVE_TRY(read_scalars(h, s, 2, st));
        const double d2 = std::sqrt((s->hscal()[0] + s->hscal()[1]) / (double)ntot) / h0;
        hstep = hw_dt1(h0, d1, d2, TT);
    } else if (!(hstep > 0)) {
        return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, "fixed-step adjoint needs opt->dt > 0");
    }
    double qold = o.qoldinit, tau = 0.0;
    size_t si = 0;
    int64_t naccept = 0, nreject = 0, it = 0;
    std::vector<double>* hrec = kanode_internal_adjoint_steps(h);
    if (hrec) hrec->clear();
    // a small chain whose steps run as one launch each: a stop's jump and FSAL re-evaluation ride in the next
    // step's launch (ChainAdjStep::fsal) instead of a launch of their own; `pend` holds them until that step
    // is accepted (a rejected attempt forms them again)
    const bool fold_stops = !s->qform && kanode_internal_chain_adjoint_step_ok(h);
    struct {
        bool on = false;
        int ng = 0;
        const void* g[8];
    } pend;
    // A step that landed on stops[si] (tau == stops[si]): the saveat jump there, if any, and the next stop.
    // k0l / k0m: the current kλ_1 / kμ_1 buffers (the FSAL re-evaluation's outputs).
    auto take_stop = [&](void* k0l, void* k0m) -> kanode_status {
        const double tsv = tf - tau;
        Jump* key = nullptr;
        for (auto& jm : jumps)
            if (jm.live && (!key || std::fabs(jm.ts - tsv) < std::fabs(key->ts - tsv))) key = &jm;
        if (key && std::fabs(key->ts - tsv) <= eps && si + 1 < stops.size()) {
            if (fold_stops && key->rows.size() <= 8) {
                pend.on = true;
                pend.ng = 0;
                for (int64_t r : key->rows) pend.g[pend.ng++] = (const char*)dl_du + r * sb;
                key->live = false;
            } else if (key->rows.size() <= (size_t)KANODE_MAX_STAGES) {
                // callback λ += ∂L/∂u(t_j) and the FSAL re-evaluation (u_modified!) as ONE adjoint
                // stage: λs = λ + Σ_r 1·g_r (the lincombs' fma order) -> λ_new, kλ_1 = λsᵀJ at λs
                void* g[KANODE_MAX_STAGES];
                double ones[KANODE_MAX_STAGES];
                int ng = 0;
                for (int64_t r : key->rows) {
                    g[ng] = (char*)dl_du + r * sb;
                    ones[ng++] = 1.0;
                }
                key->live = false;
                // (deferred where the surrogate pair's stages run lazily: its second launch then runs
                // together with the next step's first stage, whose λs starts from this kλ_1)
                SOLVE_TRY(adj_rhs(tau, lam[lcur], ng, g, ones, k0l, k0m, lam[lcur ^ 1], nullptr, nullptr,
                                  kanode_internal_pair_lazy(h)));
                lcur ^= 1;
            } else {
                SOLVE_TRY(add_jump(*key, lam[lcur]));                   // callback: λ += ∂L/∂u(t_j)
                SOLVE_TRY(adj_rhs(tau, lam[lcur], 0, nullptr, nullptr, k0l, k0m, nullptr, nullptr, nullptr));
            }
            ++nf;                                                      // u_modified!: FSAL re-evaluated
        }
        si = std::min(si + 1, stops.size() - 1);
        return KANODE_OK;
    };
    bool dev_loop = false;
    if constexpr (std::is_same<T, double>::value) {
        if (s->qform && o.adaptive && o.control == 0 && !capturing(st) && s->record) {
            double* lslab = nullptr;
            int64_t lgrid = 0;
            SOLVE_TRY(kanode_internal_fk_adjoint_loop_geometry(h, s->batch, st, dev_loop, &lslab, &lgrid));
            if (dev_loop) {
                SOLVE_TRY(adjoint_fk_loop(h, p, s, o, stops, lslab, lgrid, lam, kl, mu, km, hstep, qold, tau, si,
                                          naccept, nreject, it, nf, lcur, mcur, hrec, take_stop, st));
            }
        }
    }
    for (; !dev_loop && it < o.maxiters; ++it) {
        if (tau >= TT - 1e-14 * std::max(1.0, TT)) break;
        hstep = std::min(hstep, stops[si] - tau);
        bool fused_step = false;   // Fisher-KPP table path, Q-form dense output: the six stages in one launch
        // combined (fixed step, kanode_internal_fk_adjoint_step): the step's reduction launch reduces the
        // stage moments through the combinations the step consumes and writes μ_new itself (AdjMuUpdate)
        // and the FSAL kμ_7 into km[6]; km[1..5] are NOT written on such a step and hold stale values,
        // so nothing may read them when `combined` is set
        bool combined = false;
        bool finished = false;     // adaptive step: μ_new, kμ_7 and the μ error terms formed by the finish launch
        if (o.adaptive && s->mscal()) arm_ctl(s->hscal(), kScalars);
        lam_parts = 0;
        if (s->qform) {
            kan::AdjStepArgs a{};
            for (int j = 0; j < 7; ++j) a.kl[j] = (double*)kl[j];
            for (int i = 0; i < 6; ++i) {
                for (int j = 0; j <= i; ++j) a.a[i][j] = hstep * TA[i][j];
                const double t = tf - (i == 5 ? tau + hstep : tau + TC[i] * hstep);
                double th;
                const int64_t fi = s->locate(t, th);
                a.su_u[i] = (const double*)s->u(fi);
                for (int m = 0; m < 4; ++m) a.su_q[i][m] = (const double*)s->q(fi, m + 1);
                a.su_c[i][0] = th;
                a.su_c[i][1] = th * th;
                a.su_c[i][2] = th * th * th;
                a.su_c[i][3] = th * th * th * th;
            }
            for (int j = 0; j < 7; ++j) a.ec[j] = hstep * BT[j];
            a.abstol = o.abstol;
            a.reltol = o.reltol;
            a.lam = (const double*)lam[lcur];
            a.lam_out = (double*)lam[lcur ^ 1];
            void* kms[6] = {km[1], km[2], km[3], km[4], km[5], km[6]};
            const AdjMuUpdate mup{(const double*)mu[mcur], (double*)mu[mcur ^ 1], (const double*)km[0], hstep * TA[5][0]};
            AdjAdaptiveFinish af{};
            af.mu = (const double*)mu[mcur];
            af.mu_new = (double*)mu[mcur ^ 1];
            af.km1 = (const double*)km[0];
            af.km7 = (double*)km[6];
            for (int j = 0; j < 6; ++j) af.a6[j] = hstep * TA[5][j];
            for (int j = 0; j < 7; ++j) af.bt[j] = hstep * BT[j];
            af.abstol = o.abstol;
            af.reltol = o.reltol;
            af.out = ctl(s) + 8;
            af.done = &finished;
            SOLVE_TRY(kanode_internal_fk_adjoint_step(h, p, &a, kms, o.adaptive ? ctl(s) + 0 : nullptr, s->batch,
                                                      st, fused_step, &combined, &mup,
                                                      o.adaptive && P <= KANODE_MAX_GRID + 1 ? &af : nullptr));
        } else {
            // a small chain: the six stages in one launch (kd_chain_vjp_step_kernel), kμ_2..kμ_7 into km[1..6] and
            // the λ error into slot 0 by its reduction launch: the same values as the six adj_rhs calls below
            kan::ChainAdjStep<T> ca{};
            for (int i = 0; i < 6; ++i) {
                for (int j = 0; j < 6; ++j) ca.a[i][j] = j <= i ? hstep * TA[i][j] : 0.0;
                const double t = tf - (i == 5 ? tau + hstep : tau + TC[i] * hstep);
                double th;
                const int64_t fi = s->locate(t, th);
                const double dti = s->dts[fi];
                double c[7];
                interp_weights(th, c);
                ca.su_u[i] = (const T*)s->u(fi);
                for (int q = 0; q < 7; ++q) {
                    ca.su_k[i][q] = (const T*)s->k(fi, q + 1);
                    ca.su_c[i][q] = c[q] * dti;
                }
            }
            for (int j = 0; j < 7; ++j) ca.ec[j] = hstep * BT[j];
            ca.abstol = o.abstol;
            ca.reltol = o.reltol;
            ca.lam = (const T*)lam[lcur];
            ca.lam_out = (T*)lam[lcur ^ 1];
            ca.kl1 = (const T*)kl[0];
            ca.kl7 = (T*)kl[6];
            ca.want_error = o.adaptive ? 1 : 0;
            if (pend.on) {   // the stop's jump and kλ_1 / kμ_1 at τ (adj_rhs's dense output there)
                const double t = tf - tau;
                double th;
                const int64_t fi = s->locate(t, th);
                const double dti = s->dts[fi];
                double c[7];
                interp_weights(th, c);
                ca.fsal = 1;
                ca.njump = pend.ng;
                for (int r = 0; r < pend.ng; ++r) ca.jump[r] = (const T*)pend.g[r];
                ca.j_u = (const T*)s->u(fi);
                for (int q = 0; q < 7; ++q) {
                    ca.j_k[q] = (const T*)s->k(fi, q + 1);
                    ca.j_c[q] = c[q] * dti;
                }
            }
            void* kms[7] = {km[1], km[2], km[3], km[4], km[5], km[6], km[0]};
            SOLVE_TRY(kanode_internal_chain_adjoint_step(h, p, &ca, kms, o.adaptive ? ctl(s) + 0 : nullptr, s->batch, st,
                                                         fused_step));
            if (pend.on && !fused_step) {   // (not launched after all: the stop's own stage, as take_stop would)
                double ones[8];
                void* g[8];
                for (int r = 0; r < pend.ng; ++r) {
                    ones[r] = 1.0;
                    g[r] = const_cast<void*>(pend.g[r]);
                }
                SOLVE_TRY(adj_rhs(tau, lam[lcur], pend.ng, g, ones, kl[0], km[0], lam[lcur ^ 1], nullptr, nullptr));
                lcur ^= 1;
                pend.on = false;
            }
        }
        for (int i = 0; i < 6 && !fused_step; ++i) {
            double lc[6];
            for (int j = 0; j <= i; ++j) lc[j] = hstep * TA[i][j];
            if (i == 5) {
                double ec[7];
                for (int j = 0; j < 7; ++j) ec[j] = hstep * BT[j];
                SOLVE_TRY(adj_rhs(tau + hstep, lam[lcur], 6, kl, lc, kl[6], km[6], lam[lcur ^ 1], o.adaptive ? ec : nullptr,
                                  ctl(s) + 0, true));
            } else {
                SOLVE_TRY(adj_rhs(tau + TC[i] * hstep, lam[lcur], i + 1, kl, lc, kl[i + 1], km[i + 1], nullptr,
                                  nullptr, nullptr, true));
            }
        }
        if (!fused_step) SOLVE_TRY(kanode_internal_vjp_flush(h, st));   // km[1..6] and the λ error
        nf += 6;
        double a6[6];
        for (int j = 0; j < 6; ++j) a6[j] = hstep * TA[5][j];
        int fin_blocks = 0;
        if (combined || finished) {
            // μ_new = μ + h a_61 km_1 + (the step's combined Σ_{j>=2} h a_6j km_j): formed by the step's
            // reduction launch (kanode_internal_fk_adjoint_step: AdjMuUpdate, or AdjAdaptiveFinish)
        } else if (o.adaptive) {
            // μ_new and the μ error partials in one launch (adj_step_finish_kernel)
            kan::AdjStepFinish<T> f{};
            for (int j = 0; j < 7; ++j) {
                f.km[j] = (const T*)km[j];
                f.b[j] = hstep * BT[j];
            }
            for (int j = 0; j < 6; ++j) f.a[j] = a6[j];
            f.abstol = o.abstol;
            f.reltol = o.reltol;
            SOLVE_HIP(h, kan::launch_adj_step_finish<T>((const T*)mu[mcur], (T*)mu[mcur ^ 1], f, ctl(s) + 16, P, &fin_blocks,
                                                        st));
        } else {
            SOLVE_TRY(lincomb<T>(h, mu[mcur], 6, km, a6, mu[mcur ^ 1], P, st));   // μ_new = μ + h Σ a_6j km_j
        }
        double hnew = hstep;
        if (o.adaptive) {
            double sumsq = 0.0;
            if (finished) {   // the λ sum and the P μ terms in one read, summed here in order
                if (s->mscal()) SOLVE_TRY(wait_ctl(h, st, {{s->hscal() + 8, (int)(1 + P)}}));
                else SOLVE_TRY(read_ctl(h, s, 8, (int)(1 + P), st));
                double mus = 0.0;
                for (int64_t q = 0; q < P; ++q) mus += s->hscal()[9 + q];
                sumsq = s->hscal()[8] + mus;
            } else if (lam_parts > 0) {   // the λ error partials (hparts) and the μ partials (slots 16..)
                SOLVE_TRY(wait_ctl(h, st, {{s->hparts(), lam_parts}, {s->hscal() + 16, fin_blocks}}));
                double ls = 0.0, mus = 0.0;
                for (int b = 0; b < lam_parts; ++b) ls += s->hparts()[b];
                for (int b = 0; b < fin_blocks; ++b) mus += s->hscal()[16 + b];
                arm_ctl(s->hparts(), lam_parts);
                sumsq = ls + mus;
            } else {   // the λ total (slot 0) and the μ partials (slots 16..) in one read
                if (s->mscal()) SOLVE_TRY(wait_ctl(h, st, {{s->hscal(), 1}, {s->hscal() + 16, fin_blocks}}));
                else SOLVE_TRY(read_ctl(h, s, 0, 16 + fin_blocks, st));
                double mus = 0.0;
                for (int b = 0; b < fin_blocks; ++b) mus += s->hscal()[16 + b];
                sumsq = s->hscal()[0] + mus;
            }
            const PiStep c = pi_step(std::sqrt(sumsq / (double)ntot), hstep, qold, o);
            if (c.reject) {
                ++nreject;
                hstep = c.dt;
                continue;
            }
            hnew = c.dt;
            qold = c.qold;
        }
        tau = tau + hstep;
        lcur ^= 1;
        mcur ^= 1;
        pend.on = false;           // (the folded stop, if any, is part of this accepted step)
        std::swap(kl[0], kl[6]);   // FSAL
        std::swap(km[0], km[6]);
        if (hrec) hrec->push_back(hstep);
        ++naccept;
        if (std::fabs(tau - stops[si]) <= 1e-12 * std::max(1.0, TT)) {
            tau = stops[si];
            SOLVE_TRY(take_stop(kl[0], km[0]));
        }
        hstep = hnew;
    }
    SOLVE_TRY(kanode_internal_vjp_flush(h, st));   // (a deferred stage's last launch)
    if (pend.on) {   // (a stop no step followed: maxiters) its jump still belongs to λ
        for (int r = 0; r < pend.ng; ++r) {
            const double one = 1.0;
            SOLVE_TRY(lincomb<T>(h, lam[lcur], 1, &pend.g[r], &one, lam[lcur], n, st));
        }
    }
    if (it == o.maxiters && !(tau >= TT - 1e-14 * std::max(1.0, TT)))
        return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, "adjoint Tsit5: maxiters reached");
    for (auto& jm : jumps)   // a saveat at t0 adds to dL/du0 only
        if (jm.live && std::fabs(jm.ts - t0) <= eps) SOLVE_TRY(add_jump(jm, lam[lcur]));
    if (du0) SOLVE_HIP(h, hipMemcpyAsync(du0, lam[lcur], sb, hipMemcpyDeviceToDevice, st));
    if (dp) SOLVE_HIP(h, hipMemcpyAsync(dp, mu[mcur], pb, hipMemcpyDeviceToDevice, st));
    set_stats(stats, naccept, nreject, nf);
    return KANODE_OK;
}

}  // namespace

// The stops, saveat jump groups and options of the one-launch adjoints (adjoint_t's semantics): the jump
// groups and stops go to the solution's adj_meta buffer, everything else into a (rec, k1_0, ts, dts and
// nsteps are the caller's).
// (the groups depend on t0, tf and saveat alone, not on p: the training loop builds them once per launch)
void adjoint_jump_groups(double t0, double tf, const std::vector<double>& saveat, bool have_dl,
                         std::vector<double>& stops, std::vector<int32_t>& rows, std::vector<int32_t>& off) {
    const double TT = tf - t0;
    const double eps = 1e-12 * std::max(1.0, std::fabs(tf));
    // the jump groups of adjoint_t: distinct saveat values and their dl_du rows
    struct Jump { double ts; std::vector<int32_t> rows; };
    std::vector<Jump> jumps;
    for (int64_t jx = 0; jx < (int64_t)saveat.size(); ++jx) {
        auto f = std::find_if(jumps.begin(), jumps.end(), [&](const Jump& x) { return x.ts == saveat[jx]; });
        if (f == jumps.end()) jumps.push_back({saveat[jx], {(int32_t)jx}});
        else f->rows.push_back((int32_t)jx);
    }
    std::vector<std::pair<double, int>> st_j;   // (τ of the stop, jump)
    std::vector<int32_t> init_rows, final_rows;
    if (have_dl) {
        for (int q = 0; q < (int)jumps.size(); ++q) {
            const Jump& jm = jumps[q];
            if (jm.ts == tf) init_rows.insert(init_rows.end(), jm.rows.begin(), jm.rows.end());
            else if (t0 + eps < jm.ts && jm.ts < tf - eps) st_j.push_back({tf - jm.ts, q});
            else if (std::fabs(jm.ts - t0) <= eps) final_rows.insert(final_rows.end(), jm.rows.begin(), jm.rows.end());
        }
    }
    std::sort(st_j.begin(), st_j.end());
    stops.clear();
    rows = init_rows;
    off = {0, (int32_t)init_rows.size()};
    for (auto& x : st_j) {
        stops.push_back(x.first);
        const Jump& jm = jumps[x.second];
        const bool hit = std::fabs(jm.ts - (tf - x.first)) <= eps;
        if (hit) rows.insert(rows.end(), jm.rows.begin(), jm.rows.end());
        off.push_back((int32_t)rows.size());
    }
    stops.push_back(TT);
    rows.insert(rows.end(), final_rows.begin(), final_rows.end());
    off.push_back((int32_t)rows.size());
}

namespace {

kanode_status one_launch_adj_args(kanode_handle* h, kanode_solution* s, const void* dl_du, void* du0, void* dp,
                                  const kanode_solver_options& o, kan::ChainAdjointArgs& a, hipStream_t st) {
    if (!o.adaptive && !(o.dt > 0))
        return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, "fixed-step adjoint needs opt->dt > 0");
    const double t0 = s->t0, tf = s->tf;
    std::vector<double> stops;
    std::vector<int32_t> rows, off;
    adjoint_jump_groups(t0, tf, s->saveat, dl_du != nullptr, stops, rows, off);
    const int64_t ns = (int64_t)stops.size();
    // device copies: stops | joff | jrows
    const size_t bytes = ns * sizeof(double) + off.size() * sizeof(int32_t) + (rows.size() + 1) * sizeof(int32_t) + 64;
    auto& f = s->fused;
    if (f.adj_meta.bytes() < bytes) {
        f.meta_last.clear();   // (the device copy moves)
        SOLVE_HIP(h, f.adj_meta.reserve(bytes));
    }
    std::vector<char> host(bytes, 0);
    double* dstops = f.adj_meta.as<double>();
    int32_t* djoff = (int32_t*)(f.adj_meta.as<char>() + ns * sizeof(double));
    int32_t* djrows = djoff + off.size();
    std::memcpy(host.data(), stops.data(), ns * sizeof(double));
    std::memcpy(host.data() + ns * sizeof(double), off.data(), off.size() * sizeof(int32_t));
    if (!rows.empty())
        std::memcpy(host.data() + ns * sizeof(double) + off.size() * sizeof(int32_t), rows.data(),
                    rows.size() * sizeof(int32_t));
    SOLVE_TRY(staged_upload(h, s, f.adj_meta.ptr(), host.data(), bytes, st, &f.meta_last));
    SOLVE_HIP(h, f.out.reserve(4 * sizeof(int64_t)));
    a = kan::ChainAdjointArgs{};
    set_span_opts(a, t0, tf, o);
    a.dl_du = dl_du;
    a.stops = dstops;
    a.nstops = ns;
    a.jrows = djrows;
    a.joff = djoff;
    a.du0 = du0;
    a.dp = dp;
    a.out = f.out.as<int64_t>();
    if (kanode_internal_adjoint_steps(h)) SOLVE_TRY(adjoint_step_record(h, s, a.hs, a.hs_cap));
    return KANODE_OK;
}

// the step sizes a one-launch adjoint wrote (a.hs) into the handle's record
kanode_status fetch_adjoint_steps(kanode_handle* h, const kan::ChainAdjointArgs& a, int64_t naccept) {
    std::vector<double>* rec = kanode_internal_adjoint_steps(h);
    if (!rec || !a.hs) return KANODE_OK;
    rec->resize((size_t)std::min(naccept, a.hs_cap));
    if (!rec->empty()) SOLVE_HIP(h, hipMemcpy(rec->data(), a.hs, rec->size() * sizeof(double), hipMemcpyDeviceToHost));
    return KANODE_OK;
}

// ---- one-workgroup adjoint of a small chain (kd_chain_adjoint_kernel) ---------------------
// Needs the contiguous dense output of the one-workgroup forward solve; done = false when not
// covered (the host loop adjoint_t runs instead).
template <typename T>
kanode_status adjoint_fused_t(kanode_handle* h, const void* p, kanode_solution* s, const void* dl_du, void* du0,
                              void* dp, const kanode_solver_options& o, kanode_solve_stats* stats, hipStream_t st,
                              bool& done) {
    done = false;
    const int64_t nsteps = (int64_t)s->ts.size();
    if (o.control != 0 || capturing(st) || !s->slots_borrowed || nsteps < 1 ||
        !kanode_internal_chain_tsit5_ok(h, s->batch))
        return KANODE_OK;
    kan::ChainAdjointArgs a{};
    SOLVE_TRY(one_launch_adj_args(h, s, dl_du, du0, dp, o, a, st));
    auto& f = s->fused;
    a.rec = f.block.ptr();
    a.k1_0 = s->k1_0();
    a.ts = f.ts.as<double>();
    a.dts = f.dts(s->state_bytes());
    a.nsteps = nsteps;
    if (s->mscal()) {   // (as solve_fused_t, spinning on the counters)
        a.out = (int64_t*)s->mscal();
        arm_ctl(s->hscal(), 4);
    }
    bool launched = false;
    SOLVE_TRY(kanode_internal_chain_adjoint(h, p, s->batch, &a, st, launched));
    if (!launched) return KANODE_OK;
    if (!s->mscal()) {
        SOLVE_HIP(h, hipMemcpyAsync(s->hscal(), f.out.ptr(), 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        SOLVE_HIP(h, hipStreamSynchronize(st));
    } else {
        SOLVE_TRY(wait_ctl(h, st, {{s->hscal(), 4}}));
    }
    int64_t res[4];
    std::memcpy(res, s->hscal(), sizeof(res));
    SOLVE_TRY(finish_one_launch(h, res, stats, "adjoint Tsit5: maxiters reached"));
    SOLVE_TRY(fetch_adjoint_steps(h, a, res[0]));
    done = true;
    return KANODE_OK;
}

// ---- the persistent surrogate-pair adjoint (kd_pair_adjoint_kernel) --------------------------
// KANODE_OPT_PAIR_PERSIST: after a host-loop forward solve of an fp64 surrogate pair (K-form slots),
// the whole InterpolatingAdjoint is one launch; done = false when not covered (adjoint_t runs instead).
kanode_status adjoint_pair_t(kanode_handle* h, const void* p, kanode_solution* s, const void* dl_du, void* du0,
                             void* dp, const kanode_solver_options& o, kanode_solve_stats* stats, hipStream_t st,
                             bool& done) {
    done = false;
    const int64_t nsteps = (int64_t)s->ts.size();
    if (o.control != 0 || capturing(st) || s->slots_borrowed || s->qform || !s->record || nsteps < 1 ||
        s->dtype != KANODE_F64 || (int64_t)s->slots.size() < nsteps || !kanode_internal_pair_persist_ok(h))
        return KANODE_OK;
    const int nwg = kanode_internal_pair_adjoint_workgroups(h, s->batch);
    if (nwg < 1 || nwg > 256) return KANODE_OK;
    kan::PairAdjArgs pa{};
    SOLVE_TRY(one_launch_adj_args(h, s, dl_du, du0, dp, o, pa.c, st));
    const size_t tab = (size_t)nsteps * sizeof(double), off_tab = 256, off_ts = off_tab + tab, off_dts = off_ts + tab;
    const size_t off_x = (off_dts + tab + 255) / 256 * 256;
    const size_t need = off_x + (size_t)2 * nwg * kan::kPairAdjXW * sizeof(double);
    SOLVE_HIP(h, s->padj.reserve(need));
    std::vector<char> host(3 * tab);
    static_assert(sizeof(void*) == sizeof(double), "slot table entries are 8 bytes");
    std::memcpy(host.data(), s->slots.data(), tab);
    std::memcpy(host.data() + tab, s->ts.data(), tab);
    std::memcpy(host.data() + 2 * tab, s->dts.data(), tab);
    char* base = s->padj.as<char>();
    SOLVE_HIP(h, hipStreamSynchronize(st));   // the forward solve's kernels are done with nothing we upload
    SOLVE_HIP(h, hipMemcpy(base + off_tab, host.data(), 3 * tab, hipMemcpyHostToDevice));
    pa.c.rec = base + off_tab;
    pa.c.k1_0 = s->k1_0();
    pa.c.ts = (const double*)(base + off_ts);
    pa.c.dts = (const double*)(base + off_dts);
    pa.c.nsteps = nsteps;
    pa.ctr = (unsigned*)base;
    pa.abrt = pa.ctr + 1;
    pa.xbuf = (double*)(base + off_x);
    bool launched = false;
    SOLVE_TRY(kanode_internal_pair_adjoint(h, p, s->batch, &pa, st, launched));
    if (!launched) return KANODE_OK;
    auto& f = s->fused;
    SOLVE_HIP(h, hipMemcpyAsync(s->hscal(), f.out.ptr(), 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    unsigned abort_word = 0;
    SOLVE_HIP(h, hipMemcpyAsync(&abort_word, pa.abrt, sizeof(abort_word), hipMemcpyDeviceToHost, st));
    SOLVE_HIP(h, hipStreamSynchronize(st));
    int64_t res[4];
    std::memcpy(res, s->hscal(), sizeof(res));
    if (res[3] == 3 || abort_word != 0) {
        // an exchange timed out (workgroups not co-resident: other work held CUs) and the grid drained:
        // the launch-per-stage path (adjoint_t) re-runs the adjoint and writes every output again
        kanode_internal_set_last_adjoint(h, KANODE_ADJ_PAIR_FALLBACK);
        return KANODE_OK;
    }
    SOLVE_TRY(finish_one_launch(h, res, stats, "adjoint Tsit5: maxiters reached"));
    SOLVE_TRY(fetch_adjoint_steps(h, pa.c, res[0]));
    done = true;
    return KANODE_OK;
}

}  // namespace

extern "C" kanode_status kanode_adjoint_tsit5(kanode_handle* h, const void* p, const kanode_solution* dense,
                                              const void* dl_du, void* du0, void* dp, const kanode_solver_options* opt,
                                              kanode_solve_stats* stats, void* stream) {
    SOLVE_TRY(kanode_internal_check(h));
    const kanode_solver_options o = resolved(opt);
    SOLVE_TRY(check_opts(h, o));
    if (!p || !dense) return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, "adjoint: null p or dense output");
    kanode_solution* s = const_cast<kanode_solution*>(dense);   // scratch only; the dense output is not modified
    if (s->h != h || !s->record)
        return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, "adjoint: dense output of another handle or not recorded");
    hipStream_t st = (hipStream_t)stream;
    SOLVE_TRY(ctl_begin(h, s, st));
    TableHold hold(h);
    bool done = false;
    kanode_internal_set_last_adjoint(h, KANODE_ADJ_NONE);
    kanode_internal_clear_adjoint_steps(h);   // recorded or not: no stale sizes from an earlier adjoint
    kanode_status r = s->dtype == KANODE_F64 ? adjoint_fused_t<double>(h, p, s, dl_du, du0, dp, o, stats, st, done)
                                             : adjoint_fused_t<float>(h, p, s, dl_du, du0, dp, o, stats, st, done);
    if (r == KANODE_OK && done) kanode_internal_set_last_adjoint(h, KANODE_ADJ_CHAIN_WG);
    if (r == KANODE_OK && !done) {
        r = adjoint_pair_t(h, p, s, dl_du, du0, dp, o, stats, st, done);
        if (r == KANODE_OK && done) kanode_internal_set_last_adjoint(h, KANODE_ADJ_PAIR_PERSIST);
    }
    if (r == KANODE_OK && !done) {
        const bool fell_back = kanode_get_option(h, KANODE_OPT_LAST_ADJOINT) == KANODE_ADJ_PAIR_FALLBACK;
        r = s->dtype == KANODE_F64 ? adjoint_t<double>(h, p, s, dl_du, du0, dp, o, stats, st)
                                   : adjoint_t<float>(h, p, s, dl_du, du0, dp, o, stats, st);
        if (!fell_back) kanode_internal_set_last_adjoint(h, KANODE_ADJ_HOST_LOOP);
    }
    if (r != KANODE_OK) {
        // a failed adjoint may leave a deferred surrogate-pair stage (raw pointers into this solution and the
        // handle's workspace) and finish jobs pending on the handle: drop them, so no later call launches them
        kanode_internal_vjp_discard(h);
        s->ctl_dirty = true;
    }
    return r;
}
