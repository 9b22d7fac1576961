// kanode_train.cpp — the entry points that run whole problems in one launch around the solver's storage
// (include/kanode.h): forward sensitivities of a small Fisher-KPP field (kanode_forward_sensitivity_tsit5) and
// the two device-resident training loops (kanode_train_tsit5, kanode_train_forward_tsit5).
#include "kan_ensemble.hpp"
#include "kanode_solve_internal.hpp"

extern "C" int64_t kanode_forward_sensitivity_step_sizes(kanode_handle* h, double* ts, double* dts, int64_t cap) {
    if (!h) return -1;
    const kanode_solution* s = *(kanode_solution**)kanode_internal_solution_cache(h);
    return s ? kanode_solution_step_sizes(s, ts, dts, cap) : 0;
}

extern "C" int32_t kanode_forward_sensitivity_supported(const kanode_handle* h, int64_t batch) {
    return h && batch >= 1 && kanode_internal_fsens_ok(h, batch) ? 1 : 0;
}

extern "C" kanode_status kanode_forward_sensitivity_tsit5(kanode_handle* h, const void* p, const void* u0,
                                                           int64_t batch, double t0, double tf, const double* saveat,
                                                           int64_t n_save, void* u_save, void* s_save,
                                                           const kanode_solver_options* opt, kanode_solve_stats* stats,
                                                           void* stream) {
    SOLVE_TRY(kanode_internal_check(h));
    const kanode_solver_options o = resolved(opt);
    SOLVE_TRY(check_opts(h, o));
    if (!p || !u0 || batch < 1 || !(tf > t0) || n_save < 0 || (n_save > 0 && !saveat))
        return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, "forward sensitivities: null pointer, batch < 1 or tf <= t0");
    if (!kanode_internal_square(h))
        return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, "forward sensitivities need an RHS with N_in == N_out");
    SOLVE_TRY(check_saveat(h, saveat, n_save, tf));
    if (!kanode_internal_fsens_ok(h, batch))
        return kanode_internal_fail(h, KANODE_ERR_UNSUPPORTED,
                                    "forward sensitivities: a Fisher-KPP (pointwise + periodic Laplacian) fp64 RHS with "
                                    "nx * batch <= 64 (128 with KANODE_OPT_FSENS_WIDE), rbf basis, G = 5 or 10, base activation, softsign / tanh_fast");
    hipStream_t st = (hipStream_t)stream;
    if (capturing(st)) return kanode_internal_fail(h, KANODE_ERR_CAPTURE, "forward sensitivities read their counters");
    const int64_t n = kanode_internal_state_length(h) * batch;
    kanode_solution** slot = (kanode_solution**)kanode_internal_solution_cache(h);
    kanode_solution* s = nullptr;
    SOLVE_TRY(acquire_solution(h, slot, n, KANODE_F64, false, st, s));
    SOLVE_TRY(ctl_begin(h, s, st));
    auto& f = s->fused;
    SOLVE_TRY(upload_saveat(h, s, saveat, n_save, st));
    // the accepted step times / sizes (up to kFsensSteps), read back with the counters
    constexpr int64_t kFsensSteps = 4096;
    SOLVE_HIP(h, f.ts.reserve(2 * (size_t)kFsensSteps * sizeof(double)));
    const int64_t ts_cap = f.ts_cap();
    SOLVE_HIP(h, f.hts.reserve(f.ts.bytes()));
    double* const hts = f.hts.as<double>();
    kan::ChainSolveArgs a{};
    set_span_opts(a, t0, tf, o);
    a.cap = ts_cap;
    a.ts = f.ts.as<double>();
    a.dts = a.ts + ts_cap;
    a.n_save = n_save;
    a.saveat = f.saveat.as<double>();
    a.u_save = n_save > 0 ? u_save : nullptr;
    a.out = f.out.as<int64_t>();
    kanode_status r = kanode_internal_fk_fsens(h, p, u0, batch, &a, n_save > 0 ? s_save : nullptr, st);
    if (r != KANODE_OK) {
        s->ctl_dirty = true;
        return r;
    }
    SOLVE_HIP(h, hipMemcpyAsync(s->hscal(), a.out, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SOLVE_HIP(h, hipMemcpyAsync(hts, a.ts, 2 * (size_t)ts_cap * sizeof(double), hipMemcpyDeviceToHost, st));
    SOLVE_HIP(h, hipStreamSynchronize(st));
    int64_t res[4];
    std::memcpy(res, s->hscal(), sizeof(res));
    SOLVE_TRY(finish_one_launch(h, res, stats, "Tsit5: maxiters reached"));
    const int64_t nrec = std::min<int64_t>(res[0], ts_cap);
    s->t0 = t0;
    s->tf = tf;
    s->ts.assign(hts, hts + nrec);
    s->dts.assign(hts + ts_cap, hts + ts_cap + nrec);
    return KANODE_OK;
}

// ---- the device-resident training loop (kd_chain_train_lvsp_kernel) ---------------------------
extern "C" int32_t kanode_train_supported(const kanode_handle* h, int64_t batch) {
    return h && batch >= 1 && kanode_internal_chain_train_ok(h, batch) ? 1 : 0;
}

// The two device-resident loops share everything but the kernel: `forward` = the Fisher-KPP loop on the forward-mode
// gradient (kanode_train_forward_tsit5), else the Lotka-Volterra loop on the InterpolatingAdjoint (kanode_train_tsit5).
// ens: the ensemble entries' per-replica arrays (p, m, v and the outputs are then [R][..], iters_done and stop_reason
// [R]; eta, beta1_t, beta2_t and the handle's L1 penalty are not read), else null.  kLoopFit (with ens alone): the
// adjoint loop on the small chains that are not the Lotka-Volterra shape (kanode_fit_ensemble_tsit5).
enum TrainLoop : int { kLoopAdjoint = 0, kLoopForward = 1, kLoopFit = 2 };
static kanode_status train_tsit5_impl(TrainLoop loop, const kan::EnsembleReplicas* ens, kanode_handle* h, void* p, void* m,
                                            void* v, const void* u0, int64_t batch,
                                            double t0, double tf, const double* saveat, int64_t n_save,
                                            const void* target, double tf_test, const double* saveat_test,
                                            int64_t n_save_test, const void* target_test,
                                            const kanode_solver_options* opt, double eta, double beta1, double beta2,
                                            double eps, double beta1_t, double beta2_t, int64_t n_iters, double* loss,
                                            double* loss_test, void* grad, void* p_before, int64_t* counts,
                                            int64_t* iters_done, int32_t* stop_reason, void* stream) {
    SOLVE_TRY(kanode_internal_check(h));
    const bool forward = loop == kLoopForward, fit = loop == kLoopFit;
    const std::string name = fit ? std::string("kanode_fit_ensemble_tsit5")
                                 : std::string(forward ? "kanode_train_forward" : "kanode_train") + (ens ? "_ensemble_tsit5" : "_tsit5");
    if (fit && !ens) return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, name + ": an ensemble entry");
    if (ens && (ens->R < 1 || ens->R > kan::kTrainMaxReplicas))
        return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, name + ": 1 <= n_replicas <= 4096");
    const int64_t R = ens ? ens->R : 1;
    for (int64_t r = 0; r < R; ++r) {
        if (iters_done) iters_done[r] = 0;
        if (stop_reason) stop_reason[r] = KANODE_TRAIN_OK;
    }
    const kanode_solver_options o = resolved(opt);
    SOLVE_TRY(check_opts(h, o));
    if (fit && (batch < 1 || !kanode_internal_fit_ensemble_ok(h, batch))) {
        // (the Lotka-Volterra shape has an ensemble entry of its own, whatever KANODE_OPT_TRAIN_ANY_CHAIN says)
        const bool lv = batch >= 1 && kanode_internal_chain_train_lv_ok(h, batch);
        return kanode_internal_fail(h, KANODE_ERR_UNSUPPORTED,
                                    name + (lv ? ": not supported (one Lotka-Volterra trajectory per replica is "
                                                 "kanode_train_ensemble_tsit5's shape: call that entry)"
                                               : ": not supported (covered: every fp64 chain of the one-workgroup solve "
                                                 "and adjoint at batch <= 16 that is not the Lotka-Volterra shape, "
                                                 "fused_solve on)"));
    }
    if (!fit && !forward && (batch < 1 || !kanode_internal_chain_train_ok(h, batch)))
        return kanode_internal_fail(h, KANODE_ERR_UNSUPPORTED,
                                    name + ": not supported (covered: one trajectory of an fp64 chain [2,10,2], "
                                    "G = 5, rbf, base activations, tanh_fast / softsign, fused_solve and chain_wide on; "
                                    "with KANODE_OPT_TRAIN_ANY_CHAIN every fp64 chain of the one-workgroup solve and adjoint)");
    if (forward && (batch < 1 || !kanode_internal_fk_train_ok(h, batch, false)))
        return kanode_internal_fail(h, KANODE_ERR_UNSUPPORTED,
                                    name + ": not supported (covered: the shapes of "
                                    "kanode_forward_sensitivity_tsit5)");
    if (forward && !ens && kanode_get_l1_penalty(h) != 0.0)
        return kanode_internal_fail(h, KANODE_ERR_UNSUPPORTED,
                                    "kanode_train_forward_tsit5: not supported (the L1 penalty of "
                                    "kanode_set_l1_penalty is kanode_train_tsit5's alone; set it to 0)");
    if (ens && ens->l1)
        for (int64_t r = 0; r < R; ++r) {
            if (forward && ens->l1[r] != 0.0)
                return kanode_internal_fail(h, KANODE_ERR_UNSUPPORTED,
                                            name + ": not supported (the Fisher-KPP loop has no L1 term: l1 must be "
                                            "NULL or all zero)");
            if (!(ens->l1[r] >= 0.0 && ens->l1[r] <= 1.7976931348623157e308))
                return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, name + ": l1 must be finite and >= 0");
        }
    if (forward && n_save_test > 0 && !kanode_internal_fk_train_ok(h, batch, true))
        return kanode_internal_fail(h, KANODE_ERR_UNSUPPORTED,
                                    name + ": not supported (the test problem needs the one-workgroup "
                                    "plain solve: even nx <= 64, the table path and fused_solve on, batch <= G + 2)");
    if (ens && (!ens->eta || !ens->beta_t))
        return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, name + ": eta and beta_t are host arrays of n_replicas entries");
    if (!p || !m || !v || !u0 || !target || !loss || !saveat || n_save < 1 || n_iters < 1 || !(tf > t0) || !iters_done ||
        !stop_reason)
        return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, name + ": null pointer, n_save < 1, n_iters < 1 or tf <= t0");
    if (n_save_test < 0 || (n_save_test > 0 && (!saveat_test || !target_test || !loss_test || !(tf_test > t0))))
        return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, name + ": test problem needs saveat_test, target_test, loss_test and tf_test > t0");
    // 1 - β^t must stay positive: the bias corrections divide by it (kanode_adam_step's condition)
    for (int64_t r = 0; r < R; ++r) {
        const double b1t = ens ? ens->beta_t[2 * r] : beta1_t, b2t = ens ? ens->beta_t[2 * r + 1] : beta2_t;
        if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && b1t < 1.0 && b2t < 1.0))
            return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, name + ": Adam needs 0 <= beta < 1 and beta_t < 1");
    }
    if (check_saveat(saveat, n_save, tf, &t0) != kSaveatOk || check_saveat(saveat_test, n_save_test, tf_test, &t0) != kSaveatOk)
        return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, name + ": saveat must ascend within [t0, tf]");
    hipStream_t st = (hipStream_t)stream;
    if (capturing(st)) return kanode_internal_fail(h, KANODE_ERR_CAPTURE, name + " reads its status words");
    // the adjoint's stops and jump groups (those of kanode_adjoint_tsit5 for this saveat)
    std::vector<double> stops;
    std::vector<int32_t> rows, off;
    if (!forward) adjoint_jump_groups(t0, tf, std::vector<double>(saveat, saveat + n_save), true, stops, rows, off);
    const int64_t ns = (int64_t)stops.size();
    // (the forward loop's meta is the two saveat lists alone)
    std::vector<char> meta((size_t)(n_save + n_save_test + ns) * sizeof(double) + (off.size() + rows.size()) * sizeof(int32_t));
    {
        char* w = meta.data();
        auto put = [&](const void* src, size_t bytes) {
            if (bytes) std::memcpy(w, src, bytes);
            w += bytes;
        };
        put(saveat, (size_t)n_save * sizeof(double));
        put(saveat_test, (size_t)n_save_test * sizeof(double));
        put(stops.data(), (size_t)ns * sizeof(double));
        put(off.data(), off.size() * sizeof(int32_t));
        put(rows.data(), rows.size() * sizeof(int32_t));
    }
    kan::ChainTrainArgs a{};
    set_span_opts(a, t0, tf, o);
    a.u0 = (const double*)u0;
    a.target = (const double*)target;
    a.n_save = n_save;
    a.dl_scale = 2.0 / (double)(n_save * kanode_internal_state_length(h) * batch);
    a.nstops = ns;
    a.tf_test = tf_test;
    a.target_test = (const double*)target_test;
    a.n_save_test = n_save_test;
    a.eta = eta;
    a.ab1 = beta1;
    a.ab2 = beta2;
    a.omb1 = 1.0 - beta1;
    a.omb2 = 1.0 - beta2;
    a.eps = eps;
    a.bp1 = beta1_t;
    a.bp2 = beta2_t;
    a.n_iters = n_iters;
    a.p = (double*)p;
    a.m = (double*)m;
    a.v = (double*)v;
    a.loss = loss;
    a.loss_test = n_save_test > 0 ? loss_test : nullptr;
    a.grad = (double*)grad;
    a.p_before = (double*)p_before;
    a.counts = counts;
    a.act_reg = forward || ens ? 0.0 : kanode_get_l1_penalty(h);   // (an ensemble's: per replica, from ens->l1)
    std::vector<int64_t> res(2 * (size_t)R, 0);
    if (forward) SOLVE_TRY(kanode_internal_fk_train(h, batch, &a, ens, meta, res.data(), st));
    else if (fit) SOLVE_TRY(kanode_internal_chain_fit_ensemble(h, batch, &a, ens, meta, res.data(), st));
    else SOLVE_TRY(kanode_internal_chain_train(h, batch, &a, ens, meta, res.data(), st));
    static const char* const why[] = {"", "forward Tsit5: maxiters reached", "forward dense-output capacity exceeded "
                                      "(KANODE_OPT_FUSED_SOLVE_CAP)", "adjoint Tsit5: maxiters reached",
                                      "loss is not finite", "test-loss Tsit5: maxiters reached"};
    int64_t bad = -1;   // the lowest replica that stopped
    for (int64_t r = R - 1; r >= 0; --r) {
        iters_done[r] = res[2 * r];
        stop_reason[r] = (int32_t)res[2 * r + 1];
        if (res[2 * r + 1] != KANODE_TRAIN_OK) bad = r;
    }
    if (bad >= 0) {
        const int64_t code = res[2 * bad + 1], w = code >= 1 && code <= 5 ? code : 0;
        const kanode_status st_ = kanode_internal_fail(h, KANODE_ERR_INVALID_ARG,
                                                       name + (ens ? ": replica " + std::to_string(bad) : std::string()) +
                                                           ": stopped at iteration " + std::to_string(res[2 * bad]) +
                                                           ": " + why[w]);
        // (an ensemble launch that ran is a success: the per-replica arrays say who stopped, the text names the first)
        return ens ? KANODE_OK : st_;
    }
    return KANODE_OK;
}

extern "C" kanode_status kanode_train_tsit5(kanode_handle* h, void* p, void* m, void* v, const void* u0, int64_t batch,
                                            double t0, double tf, const double* saveat, int64_t n_save,
                                            const void* target, double tf_test, const double* saveat_test,
                                            int64_t n_save_test, const void* target_test,
                                            const kanode_solver_options* opt, double eta, double beta1, double beta2,
                                            double eps, double beta1_t, double beta2_t, int64_t n_iters, double* loss,
                                            double* loss_test, void* grad, void* p_before, int64_t* counts,
                                            int64_t* iters_done, int32_t* stop_reason, void* stream) {
    return train_tsit5_impl(kLoopAdjoint, nullptr, h, p, m, v, u0, batch, t0, tf, saveat, n_save, target, tf_test, saveat_test,
                            n_save_test, target_test, opt, eta, beta1, beta2, eps, beta1_t, beta2_t, n_iters, loss,
                            loss_test, grad, p_before, counts, iters_done, stop_reason, stream);
}

// ---- the device-resident Fisher-KPP loop on the forward-mode gradient (fk_small_train_kernel) ----
extern "C" int32_t kanode_train_forward_supported(const kanode_handle* h, int64_t batch, int32_t with_test) {
    return h && batch >= 1 && kanode_internal_fk_train_ok(h, batch, with_test != 0) ? 1 : 0;
}

extern "C" kanode_status kanode_train_forward_tsit5(kanode_handle* h, void* p, void* m, void* v, const void* u0,
                                                    int64_t batch, double t0, double tf, const double* saveat,
                                                    int64_t n_save, const void* target, double tf_test,
                                                    const double* saveat_test, int64_t n_save_test,
                                                    const void* target_test, const kanode_solver_options* opt,
                                                    double eta, double beta1, double beta2, double eps, double beta1_t,
                                                    double beta2_t, int64_t n_iters, double* loss, double* loss_test,
                                                    void* grad, void* p_before, int64_t* counts, int64_t* iters_done,
                                                    int32_t* stop_reason, void* stream) {
    return train_tsit5_impl(kLoopForward, nullptr, h, p, m, v, u0, batch, t0, tf, saveat, n_save, target, tf_test, saveat_test,
                            n_save_test, target_test, opt, eta, beta1, beta2, eps, beta1_t, beta2_t, n_iters, loss,
                            loss_test, grad, p_before, counts, iters_done, stop_reason, stream);
}

// ---- the ensemble entries: n_replicas independent loops in one launch, one workgroup each ----
static kanode_status train_ensemble(TrainLoop loop, kanode_handle* h, int64_t n_replicas, void* p, void* m, void* v,
                                    const void* u0, int64_t batch, double t0, double tf, const double* saveat,
                                    int64_t n_save, const void* target, double tf_test, const double* saveat_test,
                                    int64_t n_save_test, const void* target_test, const kanode_solver_options* opt,
                                    const double* eta, const double* l1, double beta1, double beta2, double eps,
                                    const double* beta_t, int64_t n_iters, double* loss, double* loss_test, void* grad,
                                    void* p_before, int64_t* counts, int64_t* iters_done, int32_t* stop_reason,
                                    void* stream) {
    kan::EnsembleReplicas e{};
    e.R = n_replicas;
    e.P = h ? kanode_internal_param_length(h) : 0;
    e.n_iters = n_iters;
    e.p = (double*)p;
    e.m = (double*)m;
    e.v = (double*)v;
    e.eta = eta;
    e.l1 = l1;
    e.beta_t = beta_t;
    e.loss = loss;
    e.loss_test = loss_test;
    e.grad = (double*)grad;
    e.p_before = (double*)p_before;
    e.counts = counts;
    return train_tsit5_impl(loop, &e, h, p, m, v, u0, batch, t0, tf, saveat, n_save, target, tf_test, saveat_test,
                            n_save_test, target_test, opt, 0.0, beta1, beta2, eps, 0.0, 0.0, n_iters, loss, loss_test,
                            grad, p_before, counts, iters_done, stop_reason, stream);
}

extern "C" kanode_status kanode_train_ensemble_tsit5(kanode_handle* h, int64_t n_replicas, void* p, void* m, void* v,
                                                     const void* u0, int64_t batch, double t0, double tf,
                                                     const double* saveat, int64_t n_save, const void* target,
                                                     double tf_test, const double* saveat_test, int64_t n_save_test,
                                                     const void* target_test, const kanode_solver_options* opt,
                                                     const double* eta, const double* l1, double beta1, double beta2,
                                                     double eps, const double* beta_t, int64_t n_iters, double* loss,
                                                     double* loss_test, void* grad, void* p_before, int64_t* counts,
                                                     int64_t* iters_done, int32_t* stop_reason, void* stream) {
    return train_ensemble(kLoopAdjoint, h, n_replicas, p, m, v, u0, batch, t0, tf, saveat, n_save, target, tf_test, saveat_test,
                          n_save_test, target_test, opt, eta, l1, beta1, beta2, eps, beta_t, n_iters, loss, loss_test,
                          grad, p_before, counts, iters_done, stop_reason, stream);
}

extern "C" kanode_status kanode_train_forward_ensemble_tsit5(
    kanode_handle* h, int64_t n_replicas, void* p, void* m, void* v, const void* u0, int64_t batch, double t0, double tf,
    const double* saveat, int64_t n_save, const void* target, double tf_test, const double* saveat_test,
    int64_t n_save_test, const void* target_test, const kanode_solver_options* opt, const double* eta, const double* l1,
    double beta1, double beta2, double eps, const double* beta_t, int64_t n_iters, double* loss, double* loss_test,
    void* grad, void* p_before, int64_t* counts, int64_t* iters_done, int32_t* stop_reason, void* stream) {
    return train_ensemble(kLoopForward, h, n_replicas, p, m, v, u0, batch, t0, tf, saveat, n_save, target, tf_test, saveat_test,
                          n_save_test, target_test, opt, eta, l1, beta1, beta2, eps, beta_t, n_iters, loss, loss_test,
                          grad, p_before, counts, iters_done, stop_reason, stream);
}

// ---- ensembles of the other small chains (kd_chain_train_wg_ens_kernel): the entry itself is the opt-in ----
extern "C" int32_t kanode_fit_ensemble_supported(const kanode_handle* h, int64_t batch) {
    return h && batch >= 1 && kanode_internal_fit_ensemble_ok(h, batch) ? 1 : 0;
}

extern "C" int64_t kanode_fit_ensemble_group(const kanode_handle* h, int64_t batch, double t0, double tf, int64_t n_save,
                                             int64_t n_save_test, const kanode_solver_options* opt) {
    if (!h) return 0;
    const kanode_solver_options o = resolved(opt);
    return kanode_internal_fit_ensemble_group(h, batch, o.adaptive != 0, t0, tf, o.dt, n_save, n_save_test);
}

extern "C" kanode_status kanode_fit_ensemble_tsit5(kanode_handle* h, int64_t n_replicas, void* p, void* m, void* v,
                                                   const void* u0, int64_t batch, double t0, double tf,
                                                   const double* saveat, int64_t n_save, const void* target,
                                                   double tf_test, const double* saveat_test, int64_t n_save_test,
                                                   const void* target_test, const kanode_solver_options* opt,
                                                   const double* eta, const double* l1, double beta1, double beta2,
                                                   double eps, const double* beta_t, int64_t n_iters, double* loss,
                                                   double* loss_test, void* grad, void* p_before, int64_t* counts,
                                                   int64_t* iters_done, int32_t* stop_reason, void* stream) {
    return train_ensemble(kLoopFit, h, n_replicas, p, m, v, u0, batch, t0, tf, saveat, n_save, target, tf_test,
                          saveat_test, n_save_test, target_test, opt, eta, l1, beta1, beta2, eps, beta_t, n_iters, loss,
                          loss_test, grad, p_before, counts, iters_done, stop_reason, stream);
}
