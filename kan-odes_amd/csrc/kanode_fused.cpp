// kanode_fused.cpp — what the integrator calls for one-launch steps, solves and adjoints (kanode_internal.hpp):
// whether a handle takes each of them, and the launch.  Where a launcher does not cover the shape the call returns
// OK with launched = false and the integrator runs its per-stage path.
#include "kanode.h"

#include <cstring>
#include <string>

#include "kanode_handle.hpp"

// the Fisher-KPP RHS at the reference's own sizes (kan_small.hip): one workgroup per solve / adjoint
bool fk_small_ok(const kanode_handle* h, int64_t batch) {
    return fk_table_path(h) && h->opt.fused_solve && kan::fk_small_supported(h->hlc[0], h->hpc, (int)h->spec.nx, batch);
}
kan::FkSmallArgs fk_small_args(const kanode_handle* h) {
    kan::FkSmallArgs s{};
    const FkLap lap = fk_lap(h);
    s.Nx = (int)h->spec.nx;
    s.ni = h->hpc.ni;
    s.inv_w = h->hpc.inv_w;
    s.x0 = h->hpc.x0;
    s.cd = lap.cd;
    s.co = lap.co;
    return s;
}

// ---- one Tsit5 step per launch ----
bool kanode_internal_fk_step_ok(const kanode_handle* h) {
    return fk_table_path(h) && kan::fk_stage_pp_supported(h->hpc, (int)h->spec.nx) && h->opt.fused_step;
}
bool kanode_internal_fk_loop_ok(const kanode_handle* h) { return h->opt.fk_loop && kanode_internal_fk_step_ok(h); }
kanode_status kanode_internal_fk_step_loop(kanode_handle* h, const void* p, const kan::FkLoopArgs* la, int64_t lq,
                                           int64_t batch, void* stream) {
    const hipStream_t st = (hipStream_t)stream;
    if (table_build(h, h->built_phi)) {
        const int fn_phi = kan::PP_PHI;
        HIP_TRY(h, kan::launch_fk_pp_build(h->hpc, h->dlc(), h->dpc(), (const double*)p, h->dtable(), &fn_phi, 1, st));
    }
    const auto [cd, co] = fk_lap(h);
    HIP_TRY(h, kan::launch_fk_step_pp_loop(h->hpc, h->hlc[0], h->dlc(), cd, co, (int)h->spec.nx, (const double*)p,
                                           h->dtable(), *la, lq, batch, st, h->opt.grid_rhs, &h->fk_launch));
    return KANODE_OK;
}
kanode_status kanode_internal_fk_step(kanode_handle* h, const void* p, const void* u, const void* k1,
                                      void* const* kout, void* u_new, const double* a6x6, const double* e7,
                                      const double* q4x7, double abstol, double reltol, double* err_out,
                                      int64_t batch, void* stream, bool& launched, double* err_parts,
                                      int* nparts) {
    launched = false;
    if (nparts) *nparts = 0;
    if (!kanode_internal_fk_step_ok(h)) return KANODE_OK;
    const auto [cd, co] = fk_lap(h);
    HIP_TRY(h, kan::launch_fk_step_pp(h->hpc, h->hlc[0], h->dlc(), h->dpc(), (const double*)p, h->dtable(), cd, co,
                                      (int)h->spec.nx, (const double*)u, (const double*)k1, (double* const*)kout,
                                      (double*)u_new, a6x6, e7, q4x7, abstol, reltol,
                                      err_parts && nparts ? err_parts : (double*)h->slab.ptr(), kSlabBlocks, err_out, batch,
                                      (hipStream_t)stream, table_build(h, h->built_phi), h->opt.grid_rhs,
                                      err_parts && nparts ? nparts : nullptr, &h->fk_launch));
    launched = true;
    return KANODE_OK;
}
kanode_status kanode_internal_chain_step(kanode_handle* h, const void* p, const void* u, const void* k1,
                                         void* const* kout, void* u_new, const double* a6x6, const double* e7,
                                         double abstol, double reltol, double* err_out, int64_t batch, void* stream,
                                         bool& launched) {
    launched = false;
    if (h->spec.rhs_kind != KANODE_RHS_CHAIN || !h->opt.fused_step || !all_col(h)) return KANODE_OK;
    kan::ChainStepArgs a{};
    for (int s = 0; s < 6; ++s)
        for (int j = 0; j < 6; ++j) a.a[s][j] = a6x6[6 * s + j];
    for (int j = 0; j < 7; ++j) a.e[j] = e7 ? e7[j] : 0.0;
    a.abstol = abstol;
    a.reltol = reltol;
    a.u = u;
    a.k1 = k1;
    for (int j = 0; j < 6; ++j) a.k[j] = kout[j];
    a.u_new = u_new;
    const hipError_t e = by_dtype(h, [&](auto t) {
        using T = decltype(t);
        return kan::launch_kd_chain_step<T>(h->hlc, h->n_layers, h->dlc(), (const T*)p, h->P, batch, a,
                                            (double*)h->slab.ptr(), kSlabBlocks, err_out, (hipStream_t)stream);
    });
    return launched_or_error(h, e, "launch_kd_chain_step", launched, KANODE_EVAL_CHAIN_STEP);
}

// ---- one InterpolatingAdjoint step per launch ----
// a whole InterpolatingAdjoint step of a small chain (kd_chain_vjp_step_kernel + its finish): km_out[0..5] <- kμ_2..kμ_7,
// *err_out <- the λ error total (with want_error); launched = false where the kernel does not cover the chain
template <typename T>
static kanode_status chain_adjoint_step_t(kanode_handle* h, const T* p, const kan::ChainAdjStep<T>& a,
                                          void* const* km_out, double* err_out, int64_t batch, hipStream_t st,
                                          bool& launched) {
    const size_t row = (size_t)h->P * sizeof(T) + sizeof(double);
    int64_t cap = (int64_t)(h->slab.bytes() / row) - 1;   // the stage kernel's grid cap (launch_kd_chain_vjp_stage)
    if (cap > 1024) cap = 1024;
    if (cap < 1) return KANODE_OK;
    const size_t need = kan::chain_vjp_step_slab_bytes(h->P, batch, sizeof(T), (int)cap);
    if (h->cstep_slab.bytes() < need) {
        if (is_capturing(st)) return fail(h, KANODE_ERR_CAPTURE, "chain adjoint step slab grows during capture");
        HIP_TRY(h, hipStreamSynchronize(st));
        HIP_TRY(h, h->cstep_slab.reserve(need));
    }
    T* km[7];
    for (int s = 0; s < (a.fsal ? 7 : 6); ++s) km[s] = (T*)km_out[s];
    const hipError_t e = kan::launch_kd_chain_vjp_step<T>(h->hlc, h->n_layers, h->dlc(), p, h->P, batch, a, (int)cap,
                                                          h->cstep_slab.ptr(), h->cstep_slab.bytes(), km, err_out, st);
    return launched_or_error(h, e, "launch_kd_chain_vjp_step", launched, KANODE_EVAL_CHAIN_ADJ_STEP);
}
bool kanode_internal_chain_adjoint_step_ok(const kanode_handle* h) {
    if (h->spec.rhs_kind != KANODE_RHS_CHAIN || !h->opt.fused_step || !all_col(h)) return false;
    if ((int64_t)(h->slab.bytes() / ((size_t)h->P * h->esize + sizeof(double))) - 1 < 1) return false;
    return kan::chain_vjp_step_supported(h->hlc, h->n_layers, h->P, h->esize);
}
kanode_status kanode_internal_chain_adjoint_step(kanode_handle* h, const void* p, const void* args, void* const* km_out,
                                                 double* err_out, int64_t batch, void* stream, bool& launched) {
    launched = false;
    if (!kanode_internal_chain_adjoint_step_ok(h)) return KANODE_OK;
    return by_dtype(h, [&](auto t) {
        using T = decltype(t);
        return chain_adjoint_step_t<T>(h, (const T*)p, *(const kan::ChainAdjStep<T>*)args, km_out, err_out, batch,
                                       (hipStream_t)stream, launched);
    });
}
kanode_status kanode_internal_fk_adjoint_loop_geometry(kanode_handle* h, int64_t batch, void* stream, bool& ok,
                                                      double** slab, int64_t* grid) {
    ok = false;
    if (!h->opt.fk_loop || !fk_table_path(h) || !h->opt.fused_step ||
        !kan::fk_adjoint_loop_supported(h->hpc, h->hlc[0], (int)h->spec.nx) || h->opt.grid_vstep != 0 ||
        !h->opt.vstep_rows || h->opt.adj_fused_finish || fk_moment_len(h) > KANODE_MAX_GRID + 1 ||
        kan::fk_adjoint_loop_grid(batch, kSlabBlocks / 2) < 1)
        return KANODE_OK;
    if (kanode_status s = ensure_adjoint_slabs(h, (hipStream_t)stream); s != KANODE_OK) return s;
    *slab = (double*)h->step_slab.ptr();
    *grid = kan::fk_adjoint_loop_grid(batch, kSlabBlocks / 2);
    ok = true;
    return KANODE_OK;
}
kanode_status kanode_internal_fk_adjoint_loop(kanode_handle* h, const void* p, const kan::AdjLoopArgs* la,
                                              int64_t batch, void* stream) {
    const auto [cd, co] = fk_lap(h);
    HIP_TRY(h, kan::launch_fk_adjoint_loop(h->hpc, h->hlc[0], h->dlc(), h->dpc(), (const double*)p, h->dtable(), cd, co, (int)h->spec.nx, *la, batch, (hipStream_t)stream,
                                           table_build(h, h->built_vjp), &h->fk_launch));
    return KANODE_OK;
}
kanode_status kanode_internal_fk_adjoint_step(kanode_handle* h, const void* p, kan::AdjStepArgs* a, void* const* km,
                                              double* err_out, int64_t batch, void* stream, bool& launched,
                                              bool* combined, const AdjMuUpdate* mu, const AdjAdaptiveFinish* af) {
    launched = false;
    if (combined) *combined = false;
    if (af) *af->done = false;
    if (!fk_table_path(h) || !kan::fk_vjp_pp_supported(h->hlc[0], (int)h->spec.nx) || !h->opt.fused_step)
        return KANODE_OK;
    const hipStream_t st = (hipStream_t)stream;
    const int P = fk_moment_len(h);
    if (kanode_status s = ensure_adjoint_slabs(h, st); s != KANODE_OK) return s;
    const auto [cd, co] = fk_lap(h);
    a->err_slab = err_out ? (double*)h->step_slab.ptr() : nullptr;   // relocated by the launcher
    int grid = 0, comb = 0;
    a->combine = err_out && af ? 2 : (combined != nullptr && err_out == nullptr ? 1 : 0);
    a->fin_ctr = nullptr;
    if (err_out && af && h->opt.adj_fused_finish) {   // the finish inside the rows kernel (the launcher may decline)
        a->fin_ctr = h->fin_ctr.as<unsigned>();
        a->fin = kan::AdjFinish{};
        a->fin.a0 = af->a6[0];
        a->fin.e0 = af->bt[0];
        a->fin.abstol = af->abstol;
        a->fin.reltol = af->reltol;
        a->fin.mu = af->mu;
        a->fin.mu_new = af->mu_new;
        a->fin.km1 = af->km1;
        a->fin.km7 = af->km7;
        a->fin.out = af->out;
        // the arrival counters re-zeroed on the stream before every fused launch: a wait that timed
        // out in an earlier launch cannot leave them off by one for this one
        HIP_TRY(h, hipMemsetAsync(h->fin_ctr.ptr(), 0, 2 * sizeof(unsigned), st));
    }
    bool fused_fin = false;
    HIP_TRY(h, kan::launch_fk_vjp_step_pp(h->hpc, h->hlc[0], h->dlc(), h->dpc(), (const double*)p, h->dtable(), cd, co,
                                          (int)h->spec.nx, *a, (double*)h->step_slab.ptr(), kSlabBlocks / 2, batch, &grid, st,
                                          table_build(h, h->built_vjp), h->opt.grid_vstep,
                                          h->opt.vstep_rows != 0, &comb, &fused_fin, &h->fk_launch));
    if (fused_fin) {   // μ_new, kμ_7 and the error terms are written by the step kernel itself
        *af->done = true;
        launched = true;
        return KANODE_OK;
    }
    kan::FinishJobs jobs{};
    double* base = (double*)h->step_slab.ptr();
    if (comb == 1) {
        // km[0] <- Σ_{s<5} h·a6_{s+1}·kμ_{s+2} (the kernel's combined rows), km[5] <- kμ_7
        for (int q = 0; q < 2; ++q) {
            const int s = q == 0 ? 0 : 5;
            kan::FinishJob& jb = jobs.j[q];
            jb.slab = base + (int64_t)s * grid * P;
            jb.dp = (double*)km[s];
            jb.nblk = grid;
            jb.assign = 1;
            jb.tr = 1;   // the rows kernel stores combined rows parameter-major
            if (q == 0 && mu) {   // μ_new = μ + a61·kμ_1 + A in the same launch (A itself is not stored)
                jb.dp = mu->mu_new;
                jb.base = mu->mu;
                jb.other = mu->km1;
                jb.coef = mu->a61;
            }
        }
        HIP_TRY(h, kan::launch_vjp_finish_jobs(jobs, 2, P, st));
        *combined = true;
        launched = true;
        return KANODE_OK;
    }
    if (err_out && af) {
        // adaptive step: the six stage sums, μ_new = μ + Σ h a6_j kμ_j, kμ_7 and the μ error terms in one
        // launch (slab s holds kμ_{s+2})
        kan::AdjFinish f{};
        if (comb == 2) {
            // the rows kernel reduced A = Σ_{s<5} h a6_{s+1} kμ_{s+2} (slab 0), E = Σ_s h b̃_{s+1} kμ_{s+2}
            // (slab 1) and kμ_7 (slab 5) instead of the six stage sums
            const int which[3] = {0, 1, 5};
            for (int q = 0; q < 3; ++q) {
                f.slab[q] = base + (int64_t)which[q] * grid * P;
                f.ca[q] = q == 0 ? 1.0 : 0.0;
                f.ce[q] = q == 1 ? 1.0 : 0.0;
            }
            f.nslab = 3;
            f.k7 = 2;
            f.tr = 1;   // the rows kernel stores the combined rows parameter-major
        } else {
            for (int s = 0; s < 6; ++s) {
                f.slab[s] = base + (int64_t)s * grid * P;
                f.ca[s] = s < 5 ? af->a6[s + 1] : 0.0;
                f.ce[s] = af->bt[s + 1];
            }
            f.nslab = 6;
            f.k7 = 5;
        }
        f.nblk = grid;
        f.a0 = af->a6[0];
        f.e0 = af->bt[0];
        f.abstol = af->abstol;
        f.reltol = af->reltol;
        f.mu = af->mu;
        f.mu_new = af->mu_new;
        f.km1 = af->km1;
        f.km7 = af->km7;
        f.err_slab = base + (int64_t)6 * grid * P;
        f.out = af->out;
        HIP_TRY(h, kan::launch_adj_finish(f, P, st));
        *af->done = true;
        launched = true;
        return KANODE_OK;
    }
    for (int s = 0; s < 6; ++s) {
        kan::FinishJob& jb = jobs.j[s];
        jb.slab = base + (int64_t)s * grid * P;
        jb.dp = (double*)km[s];
        jb.nblk = grid;
        jb.assign = 1;
        if (s == 5 && err_out) {
            jb.err_slab = base + (int64_t)6 * grid * P;
            jb.err_out = err_out;
        }
    }
    HIP_TRY(h, kan::launch_vjp_finish_jobs(jobs, 6, P, st));
    launched = true;
    return KANODE_OK;
}

// ---- a whole solve / adjoint per launch ----
bool kanode_internal_chain_tsit5_ok(const kanode_handle* h, int64_t batch) {
    if (fk_small_ok(h, batch)) return true;
    if (h->spec.rhs_kind != KANODE_RHS_CHAIN || batch < 1 || batch > kan::kChainSolveMaxBatch) return false;
    return h->opt.fused_solve && all_col(h);
}
kanode_status kanode_internal_chain_tsit5(kanode_handle* h, const void* p, const void* u0, int64_t batch,
                                          const kan::ChainSolveArgs* a, void* stream, bool& launched) {
    launched = false;
    const hipStream_t st = (hipStream_t)stream;
    if (fk_small_ok(h, batch)) {
        const int fn = kan::PP_PHI;
        if (table_build(h, h->built_phi))
            HIP_TRY(h, kan::launch_fk_pp_build(h->hpc, h->dlc(), h->dpc(), (const double*)p, h->dtable(), &fn, 1, st));
        const hipError_t e = kan::launch_fk_small_tsit5(h->hlc[0], h->hpc, h->dlc(), (const double*)p, h->dtable(),
                                                        fk_small_args(h), (const double*)u0, batch, *a, st);
        return launched_or_error(h, e, "launch_fk_small_tsit5", launched);
    }
    const hipError_t e = by_dtype(h, [&](auto t) {
        using T = decltype(t);
        return kan::launch_kd_chain_tsit5<T>(h->hlc, h->n_layers, h->dlc(), (const T*)p, h->P, (const T*)u0, batch, *a, st);
    });
    return launched_or_error(h, e, "launch_kd_chain_tsit5", launched);
}
kanode_status kanode_internal_chain_adjoint(kanode_handle* h, const void* p, int64_t batch,
                                            const kan::ChainAdjointArgs* a, void* stream, bool& launched) {
    launched = false;
    const hipStream_t st = (hipStream_t)stream;
    if (fk_small_ok(h, batch)) {
        const int fns[2] = {kan::PP_DPHI, kan::PP_SWISH};
        if (table_build(h, h->built_vjp))
            HIP_TRY(h, kan::launch_fk_pp_build(h->hpc, h->dlc(), h->dpc(), (const double*)p, h->dtable(), fns, 2, st));
        const hipError_t e = kan::launch_fk_small_adjoint(h->hlc[0], h->hpc, h->dlc(), (const double*)p, h->dtable(),
                                                          fk_small_args(h), batch, *a, st);
        return launched_or_error(h, e, "launch_fk_small_adjoint", launched);
    }
    const hipError_t e = by_dtype(h, [&](auto t) {
        using T = decltype(t);
        return kan::launch_kd_chain_adjoint<T>(h->hlc, h->n_layers, h->dlc(), (const T*)p, h->P, batch, *a, st,
                                               h->opt.chain_wide != 0);
    });
    return launched_or_error(h, e, "launch_kd_chain_adjoint", launched);
}
// the ensemble solve: exactly what kanode_internal_chain_tsit5 launches for (kanode_internal_chain_tsit5_ok and the
// launchers' own conditions)
bool kanode_internal_solve_ens_ok(const kanode_handle* h, int64_t batch) {
    if (!kanode_internal_chain_tsit5_ok(h, batch) || h->n_in != h->n_out) return false;
    if (fk_small_ok(h, batch)) return h->hpc.ni % kan::kPPPerBlock == 0 && h->P >= h->hlc[0].G + 1;
    return kan::chain_tsit5_ens_supported(h->hlc, h->n_layers, h->P, batch, h->esize);
}
kanode_status kanode_internal_solve_ens(kanode_handle* h, const void* p, int64_t R, const void* u0, int64_t batch,
                                        kan::ChainSolveArgs* a, const double* saveat, int64_t n_save, int64_t* res,
                                        void* stream) {
    const hipStream_t st = (hipStream_t)stream;
    const char* what = "kanode_solve_ensemble_tsit5";
    const kan::EnsSolveLayout L = kan::ens_solve_layout(R, n_save);
    const size_t res_bytes = (size_t)R * kan::kEnsSolveStatusWords * sizeof(int64_t);
    const bool fk = fk_small_ok(h, batch);
    const size_t stride = fk ? kan::ens_table_stride(kan::kPPCoef, h->hpc.ni) : 0;
    const size_t tbytes = fk ? kan::ens_table_bytes(R, kan::kPPCoef, h->hpc.ni) : 0;
    if (h->ens_solve_buf.bytes() < L.bytes || h->ens_tables.bytes() < tbytes || h->ens_solve_host.bytes() < res_bytes) {
        HIP_TRY(h, hipStreamSynchronize(st));   // (an earlier call's kernels may still use the old buffers)
        if (h->ens_solve_buf.reserve(L.bytes) != hipSuccess || h->ens_tables.reserve(tbytes) != hipSuccess ||
            h->ens_solve_host.reserve(res_bytes) != hipSuccess)
            return fail(h, KANODE_ERR_ALLOC, std::string(what) + ": out of memory for the replicas' status words and tables");
    }
    char* const base = h->ens_solve_buf.as<char>();
    // (the call synchronises before it returns, so the caller's list outlives the copy)
    HIP_TRY(h, hipMemcpyAsync(base + L.off_saveat, saveat, (size_t)n_save * sizeof(double), hipMemcpyHostToDevice, st));
    a->saveat = reinterpret_cast<const double*>(base + L.off_saveat);
    a->out = reinterpret_cast<int64_t*>(base);
    hipError_t e;
    if (fk)
        e = kan::launch_fk_small_tsit5_ens(h->hlc[0], h->hpc, h->dlc(), h->dpc(), (const double*)p, h->P,
                                           h->ens_tables.as<double>(), (int64_t)stride, fk_small_args(h),
                                           (const double*)u0, batch, *a, R, st);
    else
        e = by_dtype(h, [&](auto t) {
            using T = decltype(t);
            return kan::launch_kd_chain_tsit5_ens<T>(h->hlc, h->n_layers, h->dlc(), (const T*)p, h->P, (const T*)u0,
                                                     batch, *a, R, st);
        });
    if (e == hipErrorNotSupported) return fail(h, KANODE_ERR_UNSUPPORTED, std::string(what) + ": not supported");
    if (e != hipSuccess) return fail(h, KANODE_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    HIP_TRY(h, hipMemcpyAsync(h->ens_solve_host.ptr(), base, res_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    std::memcpy(res, h->ens_solve_host.ptr(), res_bytes);
    return KANODE_OK;
}
// the trajectory solve: a chain that kanode_internal_chain_tsit5 launches for at batch 1 (the Fisher-KPP field spends
// a wave per field, which the ensemble solve already is)
bool kanode_internal_solve_traj_ok(const kanode_handle* h) {
    if (h->spec.rhs_kind != KANODE_RHS_CHAIN || fk_small_ok(h, 1)) return false;
    if (!kanode_internal_chain_tsit5_ok(h, 1) || h->n_in != h->n_out) return false;
    return kan::chain_tsit5_traj_supported(h->hlc, h->n_layers, h->P, h->esize);
}
kanode_status kanode_internal_solve_traj(kanode_handle* h, const void* p, const void* u0, int64_t R,
                                         kan::ChainSolveArgs* a, const double* saveat, int64_t n_save, int64_t* res,
                                         void* stream) {
    const hipStream_t st = (hipStream_t)stream;
    const char* what = "kanode_solve_trajectories_tsit5";
    const kan::TrajSolveLayout L = kan::traj_solve_layout(R, n_save);
    const size_t res_bytes = kan::traj_solve_status_bytes(R);
    if (h->traj_solve_buf.bytes() < L.bytes || h->traj_solve_host.bytes() < res_bytes) {
        HIP_TRY(h, hipStreamSynchronize(st));   // (an earlier call's kernels may still use the old buffers)
        if (h->traj_solve_buf.reserve(L.bytes) != hipSuccess || h->traj_solve_host.reserve(res_bytes) != hipSuccess)
            return fail(h, KANODE_ERR_ALLOC, std::string(what) + ": out of memory for the trajectories' status words");
    }
    char* const base = h->traj_solve_buf.as<char>();
    // (the call synchronises before it returns, so the caller's list outlives the copy)
    HIP_TRY(h, hipMemcpyAsync(base + L.off_saveat, saveat, (size_t)n_save * sizeof(double), hipMemcpyHostToDevice, st));
    a->saveat = reinterpret_cast<const double*>(base + L.off_saveat);
    a->out = reinterpret_cast<int64_t*>(base);
    const hipError_t e = by_dtype(h, [&](auto t) {
        using T = decltype(t);
        return kan::launch_kd_chain_tsit5_traj<T>(h->hlc, h->n_layers, h->dlc(), (const T*)p, h->P, (const T*)u0, R, *a,
                                                  st);
    });
    if (e == hipErrorNotSupported) return fail(h, KANODE_ERR_UNSUPPORTED, std::string(what) + ": not supported");
    if (e != hipSuccess) return fail(h, KANODE_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    HIP_TRY(h, hipMemcpyAsync(h->traj_solve_host.ptr(), base, res_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    std::memcpy(res, h->traj_solve_host.ptr(), res_bytes);
    return KANODE_OK;
}

// ---- the persistent surrogate-pair adjoint ----
bool kanode_internal_pair_persist_ok(const kanode_handle* h) {
    return h->opt.pair_persist && h->spec.dtype == KANODE_F64 && h->spec.rhs_kind == KANODE_RHS_CHAIN && surrogate_pair(h);
}
int kanode_internal_pair_adjoint_workgroups(const kanode_handle* h, int64_t batch) {
    return kan::pair_adjoint_workgroups(h->hlc, batch, h->opt.pair_persist_s);
}
kanode_status kanode_internal_pair_adjoint(kanode_handle* h, const void* p, int64_t batch, kan::PairAdjArgs* a,
                                           void* stream, bool& launched) {
    launched = false;
    if (!kanode_internal_pair_persist_ok(h)) return KANODE_OK;
    a->S = h->opt.pair_persist_s;
    a->P = h->P;
    a->max_wg = h->opt.pair_persist_max_wg;
    a->force_abort = h->opt.pair_persist_abort ? 1 : 0;
    const hipError_t e = kan::launch_kd_pair_adjoint(h->hlc, h->dlc(), (const double*)p, batch, *a, (hipStream_t)stream);
    return launched_or_error(h, e, "launch_kd_pair_adjoint", launched);
}

// ---- forward sensitivities of a small Fisher-KPP field (kan_small.hip fk_small_fsens_kernel) ----
bool kanode_internal_fsens_ok(const kanode_handle* h, int64_t batch) {
    return h->spec.rhs_kind == KANODE_RHS_POINTWISE_PERIODIC_LAPLACIAN && h->spec.dtype == KANODE_F64 &&
           kan::fk_small_fsens_supported(h->hlc[0], (int)h->spec.nx, batch, h->opt.fsens_wide);
}
kanode_status kanode_internal_fk_fsens(kanode_handle* h, const void* p, const void* u0, int64_t batch,
                                       const kan::ChainSolveArgs* a, void* s_save, void* stream) {
    const hipStream_t st = (hipStream_t)stream;
    const bool tab = h->opt.pp_on && h->hpc.enabled;
    if (tab) {
        const int fns[3] = {kan::PP_PHI, kan::PP_DPHI, kan::PP_SWISH};
        HIP_TRY(h, kan::launch_fk_pp_build(h->hpc, h->dlc(), h->dpc(), (const double*)p, h->dtable(), fns, 3, st));
    }
    const hipError_t e = kan::launch_fk_small_fsens(h->hlc[0], h->hpc, tab, h->dlc(), (const double*)p,
                                                    tab ? h->dtable() : nullptr, fk_small_args(h), (const double*)u0,
                                                    batch, *a, (double*)s_save, h->opt.fsens_wide, st);
    if (e == hipErrorNotSupported)
        return fail(h, KANODE_ERR_UNSUPPORTED, "forward sensitivities: shape not covered by the one-workgroup kernel");
    if (e != hipSuccess) return fail(h, KANODE_ERR_HIP, std::string("launch_fk_small_fsens: ") + hipGetErrorString(e));
    return KANODE_OK;
}
