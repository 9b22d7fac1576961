// kanode_ens_solve.cpp — kanode_solve_ensemble_tsit5 (include/kanode.h): the forward solve of one problem at
// n_replicas parameter vectors in one launch, one workgroup per replica (kan_ens_solve.hip).  The argument checks are
// kanode_solve_tsit5's statements; the stop rule is the training ensemble's (a launch that ran is a success, the
// per-replica arrays say who stopped).
#include "kan_ensemble.hpp"
#include "kanode_solve_internal.hpp"

extern "C" int32_t kanode_solve_ensemble_supported(const kanode_handle* h, int64_t batch) {
    return h && batch >= 1 && kanode_internal_solve_ens_ok(h, batch) ? 1 : 0;
}

extern "C" kanode_status kanode_solve_ensemble_tsit5(kanode_handle* h, int64_t n_replicas, const void* p,
                                                     const void* u0, int64_t batch, double t0, double tf,
                                                     const double* saveat, int64_t n_save, void* u_save,
                                                     const kanode_solver_options* opt, kanode_solve_stats* stats,
                                                     int32_t* stop, void* stream) {
    SOLVE_TRY(kanode_internal_check(h));
    const std::string name = "kanode_solve_ensemble_tsit5";
    if (n_replicas < 1 || n_replicas > kan::kTrainMaxReplicas)
        return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, name + ": 1 <= n_replicas <= 4096");
    kanode_solver_options o = resolved(opt);
    o.control = 0;   // (not read: there is one path)
    SOLVE_TRY(check_opts(h, o));
    if (!p || !u0 || batch < 1 || !(tf > t0) || n_save < 1 || !saveat || !u_save || !stats || !stop)
        return kanode_internal_fail(h, KANODE_ERR_INVALID_ARG, name + ": null pointer, batch < 1, n_save < 1 or tf <= t0");
    SOLVE_TRY(check_saveat(h, saveat, n_save, tf));
    if (!kanode_internal_solve_ens_ok(h, batch))
        return kanode_internal_fail(h, KANODE_ERR_UNSUPPORTED,
                                    name + ": not supported (covered: what the one-workgroup solve of "
                                    "kanode_solve_tsit5 covers: chains of layers <= 16 wide at batch <= 16, and the "
                                    "Fisher-KPP field with even nx <= 64 at batch <= 16 on the fp64 table path, G = 5 or "
                                    "10, softsign / tanh_fast; fused_solve on)");
    hipStream_t st = (hipStream_t)stream;
    if (capturing(st)) return kanode_internal_fail(h, KANODE_ERR_CAPTURE, name + " reads its status words");
    kan::ChainSolveArgs a{};
    set_span_opts(a, t0, tf, o);
    a.n_save = n_save;
    a.cap = 0;   // no dense output, so no capacity stop
    a.u_save = u_save;
    std::vector<int64_t> res((size_t)n_replicas * kan::kEnsSolveStatusWords, 0);
    SOLVE_TRY(kanode_internal_solve_ens(h, p, n_replicas, u0, batch, &a, saveat, n_save, res.data(), st));
    int64_t bad = -1;   // the lowest replica that stopped
    for (int64_t r = n_replicas - 1; r >= 0; --r) {
        const int64_t* w = res.data() + kan::ens_solve_status_word(r);
        stats[r] = kanode_solve_stats{w[0], w[1], w[2]};
        stop[r] = w[3] == 0 ? KANODE_SOLVE_OK : KANODE_SOLVE_MAXITERS;
        if (w[3] != 0) bad = r;
    }
    // (a launch that ran is a success: stop[] says who stopped, the text names the first)
    if (bad >= 0)
        (void)kanode_internal_fail(h, KANODE_ERR_INVALID_ARG,
                                   name + ": replica " + std::to_string(bad) + ": Tsit5: maxiters reached");
    return KANODE_OK;
}
