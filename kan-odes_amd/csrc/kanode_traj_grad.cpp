// kanode_traj_grad.cpp — kanode_trajectories_gradient_tsit5 and its fp32 twin kanode_trajectories_gradient_f32_tsit5
// (include/kanode.h), one statement for both (trajectories_gradient<K>): the loss mean((u - target)²) over
// n_traj trajectories of one problem at one parameter vector and its gradient, every trajectory an ODE of its own
// with its own forward and adjoint step control, one workgroup each (kan_traj_grad.hip), the rows combined in a fixed
// order.  The argument checks are kanode_solve_tsit5's statements, the jump groups kanode_adjoint_tsit5's; the stop
// rule is the ensemble entries' (a call whose launches ran is a success, the per-trajectory arrays say who stopped).
#include "kan_ensemble.hpp"
#include "kanode_solve_internal.hpp"

namespace {

// what differs between the fp64 entry and the fp32 one: the argument struct, the element type and the three calls of
// kanode_train_launch.cpp
struct GradF64 {
    using Args = kan::TrajGradArgs;
    using T = double;
    static const char* name() { return "kanode_trajectories_gradient_tsit5"; }
    static const char* covered() {
        return ": not supported (covered: fp64 chains for which the one-workgroup solve of kanode_solve_tsit5 runs at "
               "batch 1 and the column-group adjoint fits: layers <= 16 wide, n_in == n_out, fused_solve on; not fp32, "
               "not the Fisher-KPP field)";
    }
    static bool ok(const kanode_handle* h) { return kanode_internal_traj_grad_ok(h); }
    static void set_p(Args& g, const void* p) { g.t.p = (double*)p; }   // (read only)
    static kanode_status run(kanode_handle* h, Args* g, int64_t R, const std::vector<char>& meta, int64_t* res,
                             double* loss, void* dp, void* st) {
        return kanode_internal_traj_grad(h, g, R, meta, res, loss, (double*)dp, st);
    }
};
struct GradF32 {
    using Args = kan::TrajGradF32Args;
    using T = float;
    static const char* name() { return "kanode_trajectories_gradient_f32_tsit5"; }
    static const char* covered() {
        return ": not supported (covered: fp32 chains for which the one-workgroup solve of kanode_solve_tsit5 runs at "
               "batch 1 and the fp32 column-group adjoint fits: layers <= 16 wide, n_in == n_out, fused_solve on, P "
               "even; not fp64, not the Fisher-KPP field)";
    }
    static bool ok(const kanode_handle* h) { return kanode_internal_traj_grad_f32_ok(h); }
    static void set_p(Args& g, const void* p) { g.p = (const float*)p; }
    static kanode_status run(kanode_handle* h, Args* g, int64_t R, const std::vector<char>& meta, int64_t* res,
                             double* loss, void* dp, void* st) {
        return kanode_internal_traj_grad_f32(h, g, R, meta, res, loss, (float*)dp, st);
    }
};

template <class K>
kanode_status trajectories_gradient(
    kanode_handle* h, const void* p, const void* u0, int64_t n_traj, double t0, double tf, const double* saveat,
    int64_t n_save, const void* target, const kanode_solver_options* opt, double* loss, void* dp, void* dp_rows,
    void* loss_rows, void* du0, void* u_save, kanode_solve_stats* fwd_stats, kanode_solve_stats* adj_stats,
    int32_t* stop, void* stream) {
    using T = typename K::T;
    SOLVE_TRY(kanode_internal_check(h));
    const std::string name = K::name();
    if (n_traj < 1 || n_traj > kan::kTrajGradMax)
        return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, name + ": 1 <= n_traj <= 65536");
    kanode_solver_options o = resolved(opt);
    o.control = 0;   // (not read: there is one path)
    SOLVE_TRY(check_opts(h, o));
    if (!p || !u0 || !(tf > t0) || n_save < 1 || !saveat || !target || !loss || !dp || !fwd_stats || !adj_stats ||
        !stop)
        return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, name + ": null pointer, n_save < 1 or tf <= t0");
    SOLVE_TRY(check_saveat(h, saveat, n_save, tf));
    if (check_saveat(saveat, n_save, tf, &t0) != kSaveatOk)
        return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, name + ": saveat must ascend within [t0, tf]");
    if (!K::ok(h)) return kanode_internal_fail(h, KANODE_ERR_UNSUPPORTED, name + K::covered());
    hipStream_t st = (hipStream_t)stream;
    if (capturing(st)) return kanode_internal_fail(h, KANODE_ERR_CAPTURE, name + " reads its status words");
    // the adjoint's stops and jump groups (those of kanode_adjoint_tsit5 for this saveat), one copy for all
    std::vector<double> stops;
    std::vector<int32_t> rows, off;
    adjoint_jump_groups(t0, tf, std::vector<double>(saveat, saveat + n_save), true, stops, rows, off);
    const int64_t ns = (int64_t)stops.size();
    std::vector<char> meta((size_t)(n_save + ns) * sizeof(double) + (off.size() + rows.size()) * sizeof(int32_t));
    {
        char* w = meta.data();
        auto put = [&](const void* src, size_t bytes) {
            if (bytes) std::memcpy(w, src, bytes);
            w += bytes;
        };
        put(saveat, (size_t)n_save * sizeof(double));
        put(stops.data(), (size_t)ns * sizeof(double));
        put(off.data(), off.size() * sizeof(int32_t));
        put(rows.data(), rows.size() * sizeof(int32_t));
    }
    typename K::Args g{};
    set_span_opts(g.t, t0, tf, o);
    K::set_p(g, p);
    g.t.n_save = n_save;
    g.t.dl_scale = 2.0 / (double)(n_save * kanode_internal_state_length(h));   // each trajectory's own MSE
    g.t.nstops = ns;
    g.t.n_iters = 1;
    g.u0 = (const T*)u0;
    g.target = (const T*)target;
    g.u_save = (T*)u_save;
    g.R_all = n_traj;
    g.dp_rows = (T*)dp_rows;
    g.loss_rows = (T*)loss_rows;
    g.du0 = (T*)du0;
    std::vector<int64_t> res((size_t)n_traj * kan::kTrajGradStatusWords, 0);
    double total = 0.0;
    SOLVE_TRY(K::run(h, &g, n_traj, meta, res.data(), &total, dp, st));
    *loss = total;
    static const char* const why[] = {"", "forward Tsit5: maxiters reached", "forward dense-output capacity exceeded "
                                      "(KANODE_OPT_FUSED_SOLVE_CAP)", "adjoint Tsit5: maxiters reached",
                                      "loss is not finite"};
    int64_t bad = -1;   // the lowest trajectory that stopped
    for (int64_t r = n_traj - 1; r >= 0; --r) {
        const int64_t* w = res.data() + kan::traj_grad_status_word(r);
        fwd_stats[r] = kanode_solve_stats{w[0], w[1], w[2]};
        adj_stats[r] = kanode_solve_stats{w[4], w[5], w[6]};
        int32_t s = KANODE_TRAIN_OK;
        if (w[3] != 0) s = w[3] == 2 ? KANODE_TRAIN_DENSE_CAPACITY : KANODE_TRAIN_FORWARD_MAXITERS;
        else if (w[7] == kan::kTrajGradAdjointSkipped) s = KANODE_TRAIN_LOSS_NOT_FINITE;
        else if (w[7] != 0) s = KANODE_TRAIN_ADJOINT_MAXITERS;
        stop[r] = s;
        if (s != KANODE_TRAIN_OK) bad = r;
    }
    // (launches that ran are a success: stop[] says who stopped, the text names the first)
    if (bad >= 0)
        (void)kanode_internal_fail(h, KANODE_ERR_INVALID_ARG,
                                   name + ": trajectory " + std::to_string(bad) + ": " + why[stop[bad]]);
    return KANODE_OK;
}

}  // namespace

extern "C" int32_t kanode_trajectories_gradient_supported(const kanode_handle* h) {
    return h && kanode_internal_traj_grad_ok(h) ? 1 : 0;
}

extern "C" int64_t kanode_trajectories_gradient_group(const kanode_handle* h, double t0, double tf, int64_t n_save,
                                                      const kanode_solver_options* opt) {
    if (!h) return 0;
    const kanode_solver_options o = resolved(opt);
    return kanode_internal_traj_grad_group(h, o.adaptive != 0, t0, tf, o.dt, n_save);
}

extern "C" kanode_status kanode_trajectories_gradient_tsit5(
    kanode_handle* h, const void* p, const void* u0, int64_t n_traj, double t0, double tf, const double* saveat,
    int64_t n_save, const void* target, const kanode_solver_options* opt, double* loss, void* dp, void* dp_rows,
    void* loss_rows, void* du0, void* u_save, kanode_solve_stats* fwd_stats, kanode_solve_stats* adj_stats,
    int32_t* stop, void* stream) {
    return trajectories_gradient<GradF64>(h, p, u0, n_traj, t0, tf, saveat, n_save, target, opt, loss, dp, dp_rows,
                                          loss_rows, du0, u_save, fwd_stats, adj_stats, stop, stream);
}

extern "C" int32_t kanode_trajectories_gradient_f32_supported(const kanode_handle* h) {
    return h && kanode_internal_traj_grad_f32_ok(h) ? 1 : 0;
}

extern "C" int64_t kanode_trajectories_gradient_f32_group(const kanode_handle* h, double t0, double tf, int64_t n_save,
                                                          const kanode_solver_options* opt) {
    if (!h) return 0;
    const kanode_solver_options o = resolved(opt);
    return kanode_internal_traj_grad_f32_group(h, o.adaptive != 0, t0, tf, o.dt, n_save);
}

extern "C" kanode_status kanode_trajectories_gradient_f32_tsit5(
    kanode_handle* h, const void* p, const void* u0, int64_t n_traj, double t0, double tf, const double* saveat,
    int64_t n_save, const void* target, const kanode_solver_options* opt, double* loss, void* dp, void* dp_rows,
    void* loss_rows, void* du0, void* u_save, kanode_solve_stats* fwd_stats, kanode_solve_stats* adj_stats,
    int32_t* stop, void* stream) {
    return trajectories_gradient<GradF32>(h, p, u0, n_traj, t0, tf, saveat, n_save, target, opt, loss, dp, dp_rows,
                                          loss_rows, du0, u_save, fwd_stats, adj_stats, stop, stream);
}
