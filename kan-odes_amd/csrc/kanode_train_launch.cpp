// kanode_train_launch.cpp — the launches of the device-resident training loops (kanode_train.cpp calls them through
// kanode_internal.hpp): the handle's training buffer, the capacity of one forward solve, and the single-replica or
// ensemble launch of the chain loops (kan_train.hip, kan_train_wg.hip) and the Fisher-KPP loop (kan_small_train.hip).
#include "kanode.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "kanode_handle.hpp"

// the Lotka-Volterra loop's shapes (kd_chain_train_lvsp_kernel): whatever KANODE_OPT_TRAIN_ANY_CHAIN says
static bool chain_train_lv_ok(const kanode_handle* h, int64_t batch) {
    return h->spec.rhs_kind == KANODE_RHS_CHAIN && kanode_internal_chain_tsit5_ok(h, batch) &&
           kan::chain_train_supported(h->hlc, h->n_layers, h->P, batch, h->esize, h->opt.chain_wide);
}
// every other small fp64 chain (kd_chain_train_wg_kernel): what kanode_train_tsit5 gains with the option on, and what
// kanode_fit_ensemble_tsit5 covers whatever the option says (never the Lotka-Volterra loop's shape)
bool kanode_internal_fit_ensemble_ok(const kanode_handle* h, int64_t batch) {
    return h->spec.dtype == KANODE_F64 && h->spec.rhs_kind == KANODE_RHS_CHAIN &&
           kanode_internal_chain_tsit5_ok(h, batch) &&
           kan::chain_train_wg_supported(h->hlc, h->n_layers, h->P, batch, h->esize, h->opt.chain_wide);
}
static bool chain_train_wg_ok(const kanode_handle* h, int64_t batch) {
    return h->opt.train_any_chain && kanode_internal_fit_ensemble_ok(h, batch);
}
bool kanode_internal_chain_train_lv_ok(const kanode_handle* h, int64_t batch) { return chain_train_lv_ok(h, batch); }
bool kanode_internal_chain_train_ok(const kanode_handle* h, int64_t batch) {
    return chain_train_lv_ok(h, batch) || chain_train_wg_ok(h, batch);
}
// The handle's training-loop buffer: result words | (the loop's private block) | meta at off_meta (an ensemble
// launch: kan_ensemble.hpp's layout, the per-replica blocks and structs before the one meta), grown on
// demand; meta is uploaded only when it differs from the last call's bytes.
static kanode_status train_buf_stage(kanode_handle* h, size_t off_meta, const std::vector<char>& meta, hipStream_t st,
                                     char*& base) {
    const size_t need = off_meta + meta.size() + 64;
    if (h->train_buf.bytes() < need) {
        HIP_TRY(h, hipStreamSynchronize(st));
        h->train_meta.clear();   // (its device copy goes)
        h->train_meta_off = 0;
        HIP_TRY(h, h->train_buf.reserve(need));
    }
    base = (char*)h->train_buf.ptr();
    if (h->train_meta != meta || h->train_meta_off != off_meta) {
        // (the earlier calls synchronised, so nothing on the device still reads the old bytes)
        HIP_TRY(h, hipMemcpy(base + off_meta, meta.data(), meta.size(), hipMemcpyHostToDevice));
        h->train_meta = meta;
        h->train_meta_off = off_meta;
    }
    return KANODE_OK;
}
// The launch of either loop once a's pointers into the single-replica buffer layout (status words at base, the
// private block at off_rec) are set, or, with ens, the ensemble launch: the buffer is laid out for ens->R replicas
// (kan_ensemble.hpp), the per-replica structs are formed from *a and uploaded with the meta, and launch(a, args, R)
// starts one workgroup per struct.  rec_bytes: a replica's private block (0: none).  Synchronises; res [R][2] =
// iterations done, stop reason of every replica.
template <class Launch>
static kanode_status train_launch(kanode_handle* h, const char* what, kan::ChainTrainArgs* a,
                                  const kan::EnsembleReplicas* ens, size_t rec_bytes, const std::vector<char>& meta,
                                  int64_t* res, hipStream_t st, Launch&& launch) {
    const int64_t R = ens ? ens->R : 1;
    kan::EnsembleLayout L{};
    if (ens) L = kan::ensemble_layout(R, rec_bytes, sizeof(kan::ChainTrainArgs));
    else {   // (the single-replica layout: result words | private block | meta)
        L.off_rec = 64;
        L.rec_stride = rec_bytes;
        L.off_args = L.off_meta = L.off_rec + rec_bytes;
    }
    char* base = nullptr;
    if (const kanode_status r = train_buf_stage(h, L.off_meta, meta, st, base); r != KANODE_OK) return r;
    const double* md = (const double*)(base + L.off_meta);
    a->saveat = md;
    a->saveat_test = md + a->n_save;
    a->stops = md + a->n_save + a->n_save_test;
    a->joff = (const int32_t*)(a->stops + a->nstops);
    a->jrows = a->joff + a->nstops + 2;
    a->rec = rec_bytes ? (double*)(base + L.off_rec) : nullptr;
    a->out = (int64_t*)base;
    const kan::ChainTrainArgs* dargs = nullptr;
    if (ens) {
        std::vector<kan::ChainTrainArgs> args((size_t)R);
        kan::ensemble_fill_args(*a, *ens, L, base, args.data());
        // (the earlier calls synchronised, so nothing on the device still reads the old structs)
        HIP_TRY(h, hipMemcpy(base + L.off_args, args.data(), args.size() * sizeof(kan::ChainTrainArgs),
                             hipMemcpyHostToDevice));
        dargs = (const kan::ChainTrainArgs*)(base + L.off_args);
    }
    const hipError_t e = launch(*a, dargs, R);
    if (e == hipErrorNotSupported)
        return fail(h, KANODE_ERR_UNSUPPORTED, std::string(what) + ": not supported (shape or saveat lists not covered "
                                                                   "by the one-workgroup training kernel)");
    if (e != hipSuccess) return fail(h, KANODE_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
    HIP_TRY(h, hipMemcpyAsync(res, base, (size_t)R * 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    return KANODE_OK;
}
// kanode_train_tsit5 on a chain that is not the Lotka-Volterra loop's (KANODE_OPT_TRAIN_ANY_CHAIN): the capacity by
// the same rules (the option, a fixed-step solve's own count, else the most steps that leave u_save / dl in LDS, at
// least 64, else kChainAdjointMaxSteps or what fits), the private block sized for it
// (one rule for a single run and for every replica of an ensemble: the same cap, dl_lds and stage_rec, so the same
// LDS carve)
struct TrainWgFit {
    int64_t cap;
    int dl_lds, stage_rec;
    size_t rec_bytes;   // the private global block (ChainTrainArgs::rec), a multiple of 64 bytes
};
// The capacity rule of the one-workgroup loops and of both trajectory gradients: KANODE_OPT_FUSED_SOLVE_CAP where set,
// else the largest capacity <= kChainAdjointMaxSteps that fits with u_save / dl in LDS (at least 64, else the largest
// that fits at all); a fixed-step solve without the option takes its own step count.  lds(cap, &dl, &sr): the launch's
// dynamic LDS at that capacity (0: no fit) and its two flags (either pointer may be null).
template <class Lds>
static bool onewg_cap_fit(const kanode_handle* h, bool adaptive, double t0, double tf, double dt, Lds&& lds,
                          int64_t& cap_out, int& dl_out, int& sr_out) {
    int64_t cap = std::min<int64_t>(h->opt.fused_solve_cap, kan::kChainAdjointMaxSteps);
    if (cap < 1) {
        auto largest = [&](bool want_dl) {   // the largest cap that fits (want_dl: with u_save / dl in LDS), 0: none
            return largest_fitting(kan::kChainAdjointMaxSteps, [&](int64_t c) {
                int dl = 0;
                return lds(c, &dl, nullptr) && (dl || !want_dl);
            });
        };
        cap = largest(true);
        if (cap < 64) cap = largest(false);
    }
    if (!adaptive && h->opt.fused_solve_cap < 1)
        cap = std::max<int64_t>(kanode_fixed_step_count(t0, tf, dt, kan::kChainAdjointMaxSteps), 1);
    int dl = 0, sr = 0;
    if (cap < 1 || !lds(cap, &dl, &sr)) return false;
    cap_out = cap;
    dl_out = dl;
    sr_out = sr;
    return true;
}
// (wide: the adjoint's model is chosen with it; the trajectory gradient passes false, the loops the handle's option)
static bool chain_train_wg_fit(const kanode_handle* h, int64_t batch, bool wide, bool adaptive, double t0, double tf,
                               double dt, int64_t n_save, int64_t n_save_test, TrainWgFit& f) {
    auto lds = [&](int64_t cap, int* dl, int* sr) {
        return kan::chain_train_wg_lds(h->hlc, h->n_layers, h->P, batch, wide, cap, n_save, n_save_test, dl, sr);
    };
    int64_t cap = 0;
    int dl = 0, sr = 0;
    if (!onewg_cap_fit(h, adaptive, t0, tf, dt, lds, cap, dl, sr)) return false;
    f.cap = cap;
    f.dl_lds = dl;
    f.stage_rec = sr;
    const size_t rec_bytes =
        sizeof(double) * kan::chain_train_wg_rec_elems((int64_t)h->n_in * batch, cap, n_save, n_save_test);
    f.rec_bytes = (rec_bytes + 63) & ~(size_t)63;
    return true;
}
// ens: the replicas of ONE launch (kanode_fit_ensemble_tsit5's group), each with a private block of its own; else
// the single run of kanode_train_tsit5
static kanode_status chain_train_wg(kanode_handle* h, const char* what, int64_t batch, kan::ChainTrainArgs* a,
                                    const kan::EnsembleReplicas* ens, const std::vector<char>& meta, int64_t* res,
                                    hipStream_t st) {
    TrainWgFit f{};
    if (!chain_train_wg_fit(h, batch, h->opt.chain_wide, a->adaptive != 0, a->t0, a->tf, a->dt, a->n_save,
                            a->n_save_test, f))
        return fail(h, KANODE_ERR_UNSUPPORTED, std::string(what) + ": not supported (the problem does not fit one workgroup's LDS)");
    const bool wide = h->opt.chain_wide;
    a->cap = f.cap;
    a->stage_rec = f.stage_rec;
    a->dl_lds = f.dl_lds;
    a->B = batch;
    a->N = h->n_in;
    return train_launch(h, what, a, ens, f.rec_bytes, meta, res, st,
                        [&](const kan::ChainTrainArgs& a0, const kan::ChainTrainArgs* dargs, int64_t R) {
                            return dargs ? kan::launch_kd_chain_train_wg_ensemble(h->hlc, h->n_layers, h->dlc(), h->P,
                                                                                  batch, wide, a0, dargs, R, st)
                                         : kan::launch_kd_chain_train_wg(h->hlc, h->n_layers, h->dlc(), h->P, batch,
                                                                         wide, a0, st);
                        });
}
int64_t kanode_internal_fit_ensemble_group(const kanode_handle* h, int64_t batch, bool adaptive, double t0, double tf,
                                           double dt, int64_t n_save, int64_t n_save_test) {
    TrainWgFit f{};
    if (batch < 1 || n_save < 1 || n_save_test < 0 || !(tf > t0) || !kanode_internal_fit_ensemble_ok(h, batch) ||
        !chain_train_wg_fit(h, batch, h->opt.chain_wide, adaptive, t0, tf, dt, n_save, n_save_test, f))
        return 0;
    return kan::ensemble_group(kan::kTrainMaxReplicas, f.rec_bytes, sizeof(kan::ChainTrainArgs),
                               kan::ensemble_meta_bound(n_save, n_save_test), kan::kEnsembleBudget);
}
kanode_status kanode_internal_chain_fit_ensemble(kanode_handle* h, int64_t batch, kan::ChainTrainArgs* a,
                                                 const kan::EnsembleReplicas* ens, const std::vector<char>& meta,
                                                 int64_t* res, void* stream) {
    const hipStream_t st = (hipStream_t)stream;
    const char* what = "kanode_fit_ensemble_tsit5";
    if (!ens || !kanode_internal_fit_ensemble_ok(h, batch))
        return fail(h, KANODE_ERR_UNSUPPORTED, std::string(what) + ": not supported");
    const int64_t G = kanode_internal_fit_ensemble_group(h, batch, a->adaptive != 0, a->t0, a->tf, a->dt, a->n_save,
                                                         a->n_save_test);
    if (G < 1)
        return fail(h, KANODE_ERR_UNSUPPORTED, std::string(what) + ": not supported (the problem does not fit one workgroup's LDS)");
    // consecutive groups of G replicas, one launch each on the stream, by the same code path (usually one group)
    for (int64_t g0 = 0; g0 < ens->R; g0 += G) {
        const kan::EnsembleReplicas e = kan::ensemble_slice(*ens, g0, G);
        if (const kanode_status r = chain_train_wg(h, what, batch, a, &e, meta, res + 2 * g0, st); r != KANODE_OK) return r;
    }
    return KANODE_OK;
}
kanode_status kanode_internal_chain_train(kanode_handle* h, int64_t batch, kan::ChainTrainArgs* a,
                                          const kan::EnsembleReplicas* ens, const std::vector<char>& meta, int64_t* res,
                                          void* stream) {
    const hipStream_t st = (hipStream_t)stream;
    const char* what = ens ? "kanode_train_ensemble_tsit5" : "kanode_train_tsit5";
    if (!chain_train_lv_ok(h, batch)) {
        if (ens || !chain_train_wg_ok(h, batch))   // (an ensemble of general chains is kanode_fit_ensemble_tsit5's)
            return fail(h, KANODE_ERR_UNSUPPORTED, std::string(what) + ": not supported (the ensemble entry covers one "
                                                                       "Lotka-Volterra trajectory per replica; "
                                                                       "kanode_fit_ensemble_tsit5 covers the other small chains)");
        return chain_train_wg(h, what, batch, a, nullptr, meta, res, st);
    }
    // the dense-output capacity of one forward solve: KANODE_OPT_FUSED_SOLVE_CAP, else the most steps whose dense
    // output still fits in LDS next to the rest (at least 64: a smaller block stays in global memory instead)
    int64_t cap = std::min<int64_t>(h->opt.fused_solve_cap, kan::kChainAdjointMaxSteps);
    if (cap < 1) {
        const int64_t staged = largest_fitting(kan::kChainAdjointMaxSteps, [&](int64_t c) {   // the largest staged cap
            int sr = 0;
            return kan::chain_train_lds(c, a->n_save, a->n_save_test, &sr) && sr;
        });
        cap = staged >= 64 ? staged : kan::kChainAdjointMaxSteps;
    }
    if (!a->adaptive && h->opt.fused_solve_cap < 1)   // fixed steps: exactly the steps of the solve (solve_fused_t's count)
        cap = std::max<int64_t>(kanode_fixed_step_count(a->t0, a->tf, a->dt, kan::kChainAdjointMaxSteps), 1);
    int stage_rec = 0;
    if (!kan::chain_train_lds(cap, a->n_save, a->n_save_test, &stage_rec))
        return fail(h, KANODE_ERR_UNSUPPORTED, std::string(what) + ": not supported (saveat lists too long for one workgroup's LDS)");
    a->cap = cap;
    a->stage_rec = stage_rec;
    // the global dense-output block: the single-replica buffer always holds the largest one (kChainAdjointMaxSteps,
    // not this launch's cap); every replica of an ensemble gets its own, of this launch's capacity, and none where
    // the dense output is staged in LDS
    const size_t rec_bytes = sizeof(double) * ((size_t)(ens ? cap : kan::kChainAdjointMaxSteps) * 7 * 2 + 2);
    return train_launch(h, what, a, ens, ens && stage_rec ? 0 : rec_bytes, meta, res, st,
                        [&](const kan::ChainTrainArgs& a0, const kan::ChainTrainArgs* dargs, int64_t R) {
                            return dargs ? kan::launch_kd_chain_train_ensemble(h->hlc, h->n_layers, h->dlc(), h->P, a0,
                                                                               dargs, R, st)
                                         : kan::launch_kd_chain_train(h->hlc, h->n_layers, h->dlc(), h->P, a0, st);
                        });
}

// ---- the trajectory gradient (kan_traj_grad.hip, kan_traj_grad_f32.hip) ----
// One statement for both element types.  TrajGradKind<T>: the argument struct, whether the handle is covered, the
// capacity and a trajectory's block, and the three launches.
template <typename T>
struct TrajGradKind;
template <>
struct TrajGradKind<double> {
    using Args = kan::TrajGradArgs;
    static const char* name() { return "kanode_trajectories_gradient_tsit5"; }
    static bool ok(const kanode_handle* h) {
        return h->spec.dtype == KANODE_F64 && h->spec.rhs_kind == KANODE_RHS_CHAIN && h->n_in == h->n_out &&
               kanode_internal_chain_tsit5_ok(h, 1) &&
               kan::chain_traj_grad_supported(h->hlc, h->n_layers, h->P, h->esize);
    }
    // the capacity by kanode_fit_ensemble_tsit5's rules at batch 1 on the ChainModel adjoint, and a trajectory's block
    static bool fit(const kanode_handle* h, bool adaptive, double t0, double tf, double dt, int64_t n_save,
                    TrainWgFit& f, size_t& block_bytes) {
        if (!chain_train_wg_fit(h, 1, false, adaptive, t0, tf, dt, n_save, 0, f) || f.stage_rec) return false;
        block_bytes = sizeof(double) * kan::traj_grad_block_elems(h->n_in, f.cap, n_save);
        return true;
    }
    static hipError_t launch(const kanode_handle* h, const Args& g, int64_t R, hipStream_t st) {
        return kan::launch_kd_chain_traj_grad(h->hlc, h->n_layers, h->dlc(), h->P, g, R, st);
    }
    static hipError_t chunks(const double* rows, int64_t R, int64_t P, double* part, hipStream_t st) {
        return kan::launch_traj_grad_chunks(rows, R, P, part, st);
    }
    static hipError_t total(const double* part, int64_t R, int64_t P, double* dp, double* loss, hipStream_t st) {
        return kan::launch_traj_grad_total(part, R, P, dp, loss, st);
    }
};
template <>
struct TrajGradKind<float> {
    using Args = kan::TrajGradF32Args;
    static const char* name() { return "kanode_trajectories_gradient_f32_tsit5"; }
    static bool ok(const kanode_handle* h) {
        return h->spec.dtype == KANODE_F32 && h->spec.rhs_kind == KANODE_RHS_CHAIN && h->n_in == h->n_out &&
               kanode_internal_chain_tsit5_ok(h, 1) && kan::chain_traj_grad_f32_supported(h->hlc, h->n_layers, h->P);
    }
    // the same capacity rule on kan_chain_plan.hpp's traj_grad_f32_lds; the block holds no gathered target
    static bool fit(const kanode_handle* h, bool adaptive, double t0, double tf, double dt, int64_t n_save,
                    TrainWgFit& f, size_t& block_bytes) {
        auto lds = [&](int64_t cap, int* dl, int* sr) {
            if (sr) *sr = 0;
            return kan::chain_traj_grad_f32_lds(h->hlc, h->n_layers, h->P, cap, n_save, dl);
        };
        if (!onewg_cap_fit(h, adaptive, t0, tf, dt, lds, f.cap, f.dl_lds, f.stage_rec)) return false;
        block_bytes = sizeof(float) * kan::traj_grad_f32_block_elems(h->n_in, f.cap, n_save);
        return true;
    }
    static hipError_t launch(const kanode_handle* h, const Args& g, int64_t R, hipStream_t st) {
        return kan::launch_kd_chain_traj_grad_f32(h->hlc, h->n_layers, h->dlc(), h->P, g, R, st);
    }
    static hipError_t chunks(const float* rows, int64_t R, int64_t P, float* part, hipStream_t st) {
        return kan::launch_traj_grad_chunks_f32(rows, R, P, part, st);
    }
    static hipError_t total(const float* part, int64_t R, int64_t P, float* dp, float* loss, hipStream_t st) {
        return kan::launch_traj_grad_total_f32(part, R, P, dp, loss, st);
    }
};
template <typename T>
static bool traj_grad_fit(const kanode_handle* h, bool adaptive, double t0, double tf, double dt, int64_t n_save,
                          TrainWgFit& f, size_t& block_bytes) {
    return n_save >= 1 && tf > t0 && TrajGradKind<T>::ok(h) &&
           TrajGradKind<T>::fit(h, adaptive, t0, tf, dt, n_save, f, block_bytes);
}
template <typename T>
static int64_t traj_grad_group(const kanode_handle* h, bool adaptive, double t0, double tf, double dt, int64_t n_save) {
    TrainWgFit f{};
    size_t block_bytes = 0;
    if (!traj_grad_fit<T>(h, adaptive, t0, tf, dt, n_save, f, block_bytes)) return 0;
    return kan::traj_grad_group_es(h->P, block_bytes, kan::traj_grad_meta_bound(n_save), kan::kEnsembleBudget, sizeof(T));
}
template <typename T>
static kanode_status traj_grad_run(kanode_handle* h, typename TrajGradKind<T>::Args* g, int64_t R,
                                   const std::vector<char>& meta, int64_t* res, double* loss, T* dp, hipStream_t st) {
    using K = TrajGradKind<T>;
    const std::string what = K::name();
    kan::ChainTrainArgs& a = g->t;
    TrainWgFit f{};
    size_t block_bytes = 0;
    if (!traj_grad_fit<T>(h, a.adaptive != 0, a.t0, a.tf, a.dt, a.n_save, f, block_bytes))
        return fail(h, KANODE_ERR_UNSUPPORTED, what + ": not supported (the problem does not fit one workgroup's LDS)");
    const size_t meta_bound = kan::traj_grad_meta_bound(a.n_save);
    const int64_t G = kan::traj_grad_group_es(h->P, block_bytes, meta_bound, kan::kEnsembleBudget, sizeof(T));
    if (G < 1 || meta.size() > meta_bound)
        return fail(h, KANODE_ERR_UNSUPPORTED, what + ": not supported (a launch group does not fit the handle's buffer)");
    const int64_t Gn = std::min(R, G);
    const kan::TrajGradLayout L = kan::traj_grad_layout_es(R, Gn, h->P, block_bytes, meta.size(), sizeof(T));
    const size_t host_bytes = kan::traj_grad_host_bytes(R);
    if (h->traj_grad_buf.bytes() < L.bytes || h->traj_grad_host.bytes() < host_bytes) {
        HIP_TRY(h, hipStreamSynchronize(st));   // (an earlier call's kernels may still use the old buffers)
        if (h->traj_grad_buf.reserve(L.bytes) != hipSuccess || h->traj_grad_host.reserve(host_bytes) != hipSuccess)
            return fail(h, KANODE_ERR_ALLOC, what + ": out of memory for the trajectories' blocks");
    }
    char* const base = h->traj_grad_buf.as<char>();
    // (the call synchronises before it returns, so the caller's bytes outlive the copy)
    HIP_TRY(h, hipMemcpyAsync(base + L.off_meta, meta.data(), meta.size(), hipMemcpyHostToDevice, st));
    const double* md = (const double*)(base + L.off_meta);
    a.saveat = md;
    a.saveat_test = nullptr;
    a.stops = md + a.n_save;
    a.joff = (const int32_t*)(a.stops + a.nstops);
    a.jrows = a.joff + a.nstops + 2;
    a.cap = f.cap;
    a.dl_lds = f.dl_lds;
    a.stage_rec = 0;
    a.B = 1;
    a.N = h->n_in;
    const typename K::Args all = *g;
    const size_t N = (size_t)h->n_in, P = (size_t)h->P;
    T* const part = (T*)(base + L.off_part);
    T* const dloss = (T*)(base + L.off_loss);
    // consecutive groups of G trajectories, one launch and its chunk sums each, in stream order (they share the
    // rows and the blocks); G is a multiple of the chunk, so a group's chunks are whole
    for (int64_t g0 = 0; g0 < R; g0 += G) {
        const int64_t Rg = std::min(G, R - g0);
        typename K::Args gg = all;
        gg.u0 = all.u0 + (size_t)g0 * N;
        gg.target = all.target + (size_t)g0 * N;
        gg.u_save = all.u_save ? all.u_save + (size_t)g0 * N : nullptr;
        gg.R_all = R;
        gg.blocks = base + L.off_blocks;
        gg.block_stride = L.block_stride;
        gg.rows = (T*)(base + L.off_rows);
        gg.dp_rows = all.dp_rows ? all.dp_rows + (size_t)g0 * P : nullptr;
        gg.loss_rows = all.loss_rows ? all.loss_rows + g0 : nullptr;
        gg.du0 = all.du0 ? all.du0 + (size_t)g0 * N : nullptr;
        gg.status = (int64_t*)base + kan::traj_grad_status_word(g0);
        hipError_t e = K::launch(h, gg, Rg, st);
        if (e == hipErrorNotSupported)
            return fail(h, KANODE_ERR_UNSUPPORTED, what + ": not supported (shape or saveat list not covered by the "
                                                          "one-workgroup kernel)");
        if (e == hipSuccess)
            e = K::chunks(gg.rows, Rg, h->P,
                          part + (size_t)(g0 / kan::kTrajGradChunk) * kan::traj_grad_row_elems(h->P), st);
        if (e != hipSuccess) return fail(h, KANODE_ERR_HIP, what + " launch: " + hipGetErrorString(e));
    }
    if (const hipError_t e = K::total(part, R, h->P, dp, dloss, st); e != hipSuccess)
        return fail(h, KANODE_ERR_HIP, what + " reduction: " + hipGetErrorString(e));
    HIP_TRY(h, hipMemcpyAsync(h->traj_grad_host.ptr(), base, host_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    const char* hp = h->traj_grad_host.as<char>();
    std::memcpy(res, hp, (size_t)R * kan::kTrajGradStatusWords * sizeof(int64_t));
    T total = T(0);
    std::memcpy(&total, hp + L.off_loss, sizeof(T));
    *loss = (double)total;
    return KANODE_OK;
}
bool kanode_internal_traj_grad_ok(const kanode_handle* h) { return TrajGradKind<double>::ok(h); }
int64_t kanode_internal_traj_grad_group(const kanode_handle* h, bool adaptive, double t0, double tf, double dt,
                                        int64_t n_save) {
    return traj_grad_group<double>(h, adaptive, t0, tf, dt, n_save);
}
kanode_status kanode_internal_traj_grad(kanode_handle* h, kan::TrajGradArgs* g, int64_t R,
                                        const std::vector<char>& meta, int64_t* res, double* loss, double* dp,
                                        void* stream) {
    return traj_grad_run<double>(h, g, R, meta, res, loss, dp, (hipStream_t)stream);
}
bool kanode_internal_traj_grad_f32_ok(const kanode_handle* h) { return TrajGradKind<float>::ok(h); }
int64_t kanode_internal_traj_grad_f32_group(const kanode_handle* h, bool adaptive, double t0, double tf, double dt,
                                            int64_t n_save) {
    return traj_grad_group<float>(h, adaptive, t0, tf, dt, n_save);
}
kanode_status kanode_internal_traj_grad_f32(kanode_handle* h, kan::TrajGradF32Args* g, int64_t R,
                                            const std::vector<char>& meta, int64_t* res, double* loss, float* dp,
                                            void* stream) {
    return traj_grad_run<float>(h, g, R, meta, res, loss, dp, (hipStream_t)stream);
}

bool kanode_internal_fk_train_ok(const kanode_handle* h, int64_t batch, bool with_test) {
    if (!kanode_internal_fsens_ok(h, batch) || (with_test && !fk_small_ok(h, batch))) return false;
    return kan::fk_small_train_supported(h->hlc[0], h->hpc, h->opt.pp_on && h->hpc.enabled, (int)h->spec.nx, batch,
                                         h->opt.fsens_wide, with_test);
}
kanode_status kanode_internal_fk_train(kanode_handle* h, int64_t batch, kan::ChainTrainArgs* a,
                                       const kan::EnsembleReplicas* ens, const std::vector<char>& meta, int64_t* res,
                                       void* stream) {
    const hipStream_t st = (hipStream_t)stream;
    const char* what = ens ? "kanode_train_forward_ensemble_tsit5" : "kanode_train_forward_tsit5";
    // the accumulators of the two-entries-per-lane kernel (ChainTrainArgs::rec; launch_fk_small_fsens's rule): every
    // replica of an ensemble has its own block, and none where the kernel keeps them in LDS
    const bool two = h->opt.fsens_wide == 2 || h->spec.nx * batch > 64;
    const size_t rec_bytes = sizeof(double) * (size_t)kan::kFsensMaxWaves * 2 * 64;
    const bool tab = h->opt.pp_on && h->hpc.enabled;
    return train_launch(h, what, a, ens, ens && !two ? 0 : rec_bytes, meta, res, st,
                        [&](const kan::ChainTrainArgs& a0, const kan::ChainTrainArgs* dargs, int64_t R) {
                            return dargs ? kan::launch_fk_small_train_ensemble(h->hlc[0], h->hpc, tab, h->dlc(), h->dpc(),
                                                                               fk_small_args(h), batch, a0, dargs, R,
                                                                               h->opt.fsens_wide, st)
                                         : kan::launch_fk_small_train(h->hlc[0], h->hpc, tab, h->dlc(), h->dpc(),
                                                                      fk_small_args(h), batch, a0, h->opt.fsens_wide, st);
                        });
}
