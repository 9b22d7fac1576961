// kanode_traj_solve.cpp — kanode_solve_trajectories_tsit5 (include/kanode.h): the forward solves of one problem at one
// parameter vector from n_traj initial conditions in one launch, every trajectory an ODE of its own on a 16-lane
// row (kan_traj_solve.hip).  The argument checks are kanode_solve_tsit5's statements; the stop rule is the ensemble
// solve's (a launch that ran is a success, the per-trajectory arrays say who stopped).
#include "kan_ensemble.hpp"
#include "kanode_solve_internal.hpp"

extern "C" int32_t kanode_solve_trajectories_supported(const kanode_handle* h) {
    return h && kanode_internal_solve_traj_ok(h) ? 1 : 0;
}

extern "C" kanode_status kanode_solve_trajectories_tsit5(kanode_handle* h, const void* p, const void* u0,
                                                         int64_t n_traj, double t0, double tf, const double* saveat,
                                                         int64_t n_save, void* u_save,
                                                         const kanode_solver_options* opt, kanode_solve_stats* stats,
                                                         int32_t* stop, void* stream) {
    SOLVE_TRY(kanode_internal_check(h));
    const std::string name = "kanode_solve_trajectories_tsit5";
    if (n_traj < 1 || n_traj > kan::kTrajMaxTrajectories)
        return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, name + ": 1 <= n_traj <= 65536");
    kanode_solver_options o = resolved(opt);
    o.control = 0;   // (not read: there is one path)
    SOLVE_TRY(check_opts(h, o));
    if (!p || !u0 || !(tf > t0) || n_save < 1 || !saveat || !u_save || !stats || !stop)
        return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, name + ": null pointer, n_save < 1 or tf <= t0");
    SOLVE_TRY(check_saveat(h, saveat, n_save, tf));
    if (!kanode_internal_solve_traj_ok(h))
        return kanode_internal_fail(h, KANODE_ERR_UNSUPPORTED,
                                    name + ": not supported (covered: chains for which the one-workgroup solve of "
                                    "kanode_solve_tsit5 runs at batch 1: layers <= 16 wide, n_in == n_out, fused_solve "
                                    "on; not the Fisher-KPP field)");
    hipStream_t st = (hipStream_t)stream;
    if (capturing(st)) return kanode_internal_fail(h, KANODE_ERR_CAPTURE, name + " reads its status words");
    kan::ChainSolveArgs a{};
    set_span_opts(a, t0, tf, o);
    a.n_save = n_save;
    a.cap = 0;   // no dense output, so no capacity stop
    a.u_save = u_save;
    std::vector<int64_t> res((size_t)n_traj * kan::kTrajSolveStatusWords, 0);
    SOLVE_TRY(kanode_internal_solve_traj(h, p, u0, n_traj, &a, saveat, n_save, res.data(), st));
    int64_t bad = -1;   // the lowest trajectory that stopped
    for (int64_t r = n_traj - 1; r >= 0; --r) {
        const int64_t* w = res.data() + kan::traj_solve_status_word(r);
        stats[r] = kanode_solve_stats{w[0], w[1], w[2]};
        stop[r] = w[3] == 0 ? KANODE_SOLVE_OK : KANODE_SOLVE_MAXITERS;
        if (w[3] != 0) bad = r;
    }
    // (a launch that ran is a success: stop[] says who stopped, the text names the first)
    if (bad >= 0)
        (void)kanode_internal_fail(h, KANODE_ERR_INVALID_ARG,
                                   name + ": trajectory " + std::to_string(bad) + ": Tsit5: maxiters reached");
    return KANODE_OK;
}
