// kanode_handle.hpp — struct kanode_handle and the small statements every translation unit that touches its fields
// shares (kanode_abi.cpp, kanode_eval.cpp, kanode_fused.cpp, kanode_train_launch.cpp).  C++ linkage, private to the
// library, not installed; the integrator files see the handle only through kanode_internal.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

#include "kan_buf.hpp"
#include "kan_device.hpp"
#include "kan_ensemble.hpp"
#include "kan_kernels.hpp"
#include "kanode_internal.hpp"
#include "kanode_options.hpp"   // kSlabBlocks, HandleOptions

using kan::LayerConst;

// column: thread per batch column (small I·G, O <= 16; e.g. LV [2,10,2]);
// wide-in / wide-out: the surrogate shapes (kan_wide.hip)
enum LayerKind { KIND_COL = 0, KIND_WIDE_IN = 1, KIND_WIDE_OUT = 2 };

struct kanode_handle {
    kanode_spec spec{};
    int n_layers = 0;
    LayerConst hlc[KANODE_MAX_LAYERS];
    LayerKind kind[KANODE_MAX_LAYERS];
    kan::DevBuf dlc_buf;              // device copy
    LayerConst* dlc() const { return dlc_buf.as<LayerConst>(); }
    int64_t P = 0;
    int64_t n_in = 0, n_out = 0;      // state length (input / output of the RHS)
    size_t esize = 8;
    int max_layer_P = 0;
    int max_dim = 0;
    // workspaces (device)
    kan::DevBuf slab;
    kan::DevBuf ws;                   // chain activations / gradients
    int64_t reserved_batch = 0;
    // piecewise-polynomial pointwise RHS (kan_pp.hip)
    kan::PPConst hpc{};
    kan::DevBuf dpc_buf, dtable_buf;
    kan::PPConst* dpc() const { return dpc_buf.as<kan::PPConst>(); }
    double* dtable() const { return dtable_buf.as<double>(); }
    HandleOptions opt;                // kanode_set_option (kanode_options.hpp)
    kan::FkLaunchRec fk_launch{};     // the last table launch (kanode_last_fk_launch; family 0: none yet)
    double l1_penalty = 0.0;          // kanode_set_l1_penalty: λ of kanode_train_tsit5's loss term λ·Σ|p|
    std::vector<double> adj_steps;    // the last kanode_adjoint_tsit5's accepted step sizes (when recorded)
    kan::DevBuf fin_ctr;              // ADJ_FUSED_FINISH's two arrival counters (unsigned, zeroed at allocation)
    // the surrogate pair's deferred adjoint stage: its second launch, held until the next stage is issued
    // (then both run as kd_vjp_pair_ba_kernel) or kanode_internal_vjp_flush; pair_par picks the buffers of
    // the ping-pong pairs (hidden / dot-product partials, basis store, y, λs) the next stage writes
    kan::PairPlan<double> pend_d{};
    kan::PairPlan<float> pend_f{};
    bool pend_valid = false;
    int pair_par = 0;
    // (set by the integrator) a lazy pair stage's λ error as per-block partials in err_parts (mapped host
    // memory, summed by the host), their count in *err_nparts, instead of a final-reduction launch
    double* err_parts = nullptr;
    int* err_nparts = nullptr;
    // the integrator's storage for solves without a dense output (kanode_solve.cpp)
    kanode_solution* solve_cache = nullptr;
    // the device-resident training loop (kanode_train_tsit5): result words | dense-output block | meta, and the
    // meta bytes last uploaded
    kan::DevBuf train_buf;
    std::vector<char> train_meta;
    size_t train_meta_off = 0;        // where in train_buf those bytes lie
    // the ensemble solve (kanode_solve_ensemble_tsit5; kan_ensemble.hpp): status words | saveat, the host copy of
    // the status words, and one PP_PHI table per replica (not dtable: that one, its stamps and built_phi stay as
    // the single-replica paths left them).  Grow-only; kanode_reserve does not cover them.
    kan::DevBuf ens_solve_buf, ens_tables;
    kan::PinnedBuf ens_solve_host;
    // the trajectory solve (kanode_solve_trajectories_tsit5; kan_ensemble.hpp): status words | saveat, and the host
    // copy of the status words.  Grow-only; kanode_reserve does not cover them.
    kan::DevBuf traj_solve_buf;
    kan::PinnedBuf traj_solve_host;
    // the trajectory gradient (kanode_trajectories_gradient_tsit5; kan_ensemble.hpp's TrajGradLayout), and the host
    // copy of its status words and loss.  Grow-only, at most kEnsembleBudget; kanode_reserve does not cover them.
    kan::DevBuf traj_grad_buf;
    kan::PinnedBuf traj_grad_host;
    // table reuse inside one integrator solve (p constant): build each table set once
    bool hold_tables = false;
    bool built_phi = false, built_vjp = false;
    // adjoint stages whose dp / error reductions wait for kanode_internal_vjp_flush (one launch)
    kan::DevBuf defer_slab;
    kan::DevBuf cstep_slab;           // the fused small-chain adjoint step's six stage regions (grown on demand)
    kan::DevBuf step_slab;            // fused adjoint step: six stages' moment rows + error partials
    kan::FinishJobs jobs{};
    int njobs = 0;
    // stage input y for kanode_rhs_stage's unfused path
    kan::DevBuf stage_ws;
    // host staging (device buffers) for *_host calls
    kan::DevBuf stage;
    std::string err;
};

// (nothing below is part of the library's dynamic symbol table)
#pragma GCC visibility push(hidden)

inline kanode_status fail(kanode_handle* h, kanode_status s, const std::string& msg) {
    if (h) h->err = msg;
    return s;
}

#define HIP_TRY(h, expr)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail((h), KANODE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

inline kanode_status check_handle(kanode_handle* h) {
    if (!h) return KANODE_ERR_INVALID_ARG;
    hipError_t e = hipSetDevice(h->spec.device);
    if (e != hipSuccess) return fail(h, KANODE_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    return KANODE_OK;
}

// true when the launch must (re)build its table set; under hold_tables only the first does
inline bool table_build(kanode_handle* h, bool& built) {
    if (!h->hold_tables) return true;
    if (built) return false;
    built = true;
    return true;
}

inline bool is_capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) return false;
    return cs != hipStreamCaptureStatusNone;
}

// f(double{}) or f(float{}) by the dtype: a generic lambda takes T from its argument and does the casts
template <class F>
inline auto by_dtype(int dtype, F&& f) {
    return dtype == KANODE_F64 ? f(double{}) : f(float{});
}
template <class F>
inline auto by_dtype(const kanode_handle* h, F&& f) {
    return by_dtype((int)h->spec.dtype, std::forward<F>(f));
}

// KANODE_OPT_LAST_EVAL: the launcher that served this evaluation call (a kanode_eval_path value)
inline void served(kanode_handle* h, kanode_eval_path path) { h->opt.last_eval = path; }

// A launcher's answer: hipSuccess sets launched (and records `path` where the caller names one);
// hipErrorNotSupported means "not covered, the caller falls back" (OK, launched untouched); anything else is an
// error named after the launcher.  No message is built otherwise.
inline kanode_status launched_or_error(kanode_handle* h, hipError_t e, const char* what, bool& launched,
                                       kanode_eval_path path = KANODE_EVAL_NONE) {
    if (e == hipSuccess) {
        launched = true;
        if (path != KANODE_EVAL_NONE) served(h, path);
        return KANODE_OK;
    }
    if (e == hipErrorNotSupported) return KANODE_OK;
    return fail(h, KANODE_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// every layer runs the column kernels (the one-launch small-chain kernels' first condition)
inline bool all_col(const kanode_handle* h) {
    for (int l = 0; l < h->n_layers; ++l)
        if (h->kind[l] != KIND_COL) return false;
    return true;
}

// The full-field surrogate shape KAN [N, H, N] (Burgers_Surrogate.jl:85-88,
// Schrodinger_Surrogate.jl:93-96): a wide-in layer feeding a wide-out layer.  Its RHS and VJP
// hand the hidden layer over as the wide-in chunk partials (no reduce launch).
inline bool surrogate_pair(const kanode_handle* h) {
    return h->n_layers == 2 && h->kind[0] == KIND_WIDE_IN && h->kind[1] == KIND_WIDE_OUT;
}

// the Fisher-KPP table path's common condition; every site adds its own tail (the kernel's _supported, fused_step, ...)
inline bool fk_table_path(const kanode_handle* h) {
    return h->spec.dtype == KANODE_F64 && h->spec.rhs_kind == KANODE_RHS_POINTWISE_PERIODIC_LAPLACIAN && h->opt.pp_on;
}

// the periodic Laplacian's coefficients D·(−2/dx²) (diagonal) and D·(1/dx²) (off-diagonal)
struct FkLap {
    double cd, co;
};
inline FkLap fk_lap(const kanode_handle* h) {
    const double dx2 = h->spec.dx * h->spec.dx;
    return {h->spec.diffusion * (-2.0 / dx2), h->spec.diffusion * (1.0 / dx2)};
}

// length of a Fisher-KPP moment row: the G basis coefficients and, with it, the base activation's weight
inline int fk_moment_len(const kanode_handle* h) { return h->hlc[0].G + (h->hlc[0].use_base ? 1 : 0); }

// ---- shared between the translation units ----
// kanode_eval.cpp: workspaces (never grown under capture), the pending adjoint-stage launches / reductions
kanode_status ensure_ws(kanode_handle* h, int64_t B, hipStream_t st);
kanode_status ensure_fk_ws(kanode_handle* h, int64_t B, hipStream_t st);
kanode_status ensure_stage_ws(kanode_handle* h, size_t need, hipStream_t st);
kanode_status ensure_adjoint_slabs(kanode_handle* h, hipStream_t st, bool at_create = false);
kanode_status flush_pair(kanode_handle* h, hipStream_t st);
kanode_status vjp_flush(kanode_handle* h, hipStream_t st);
// kanode_fused.cpp: the Fisher-KPP RHS at the reference's own sizes (kan_small.hip), one workgroup per solve / adjoint
bool fk_small_ok(const kanode_handle* h, int64_t batch);
kan::FkSmallArgs fk_small_args(const kanode_handle* h);

#pragma GCC visibility pop
