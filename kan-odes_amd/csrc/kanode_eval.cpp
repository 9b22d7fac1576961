// kanode_eval.cpp — the evaluation paths of a handle: the chain workspace, the RHS, its VJP, the Runge-Kutta stage
// and the adjoint stage (each templated on the dtype), the public entry points that dispatch into them and the
// integrator's twins of those entry points (kanode_internal.hpp).
#include "kanode.h"

#include <algorithm>
#include <string>
#include <type_traits>

#include "kanode_handle.hpp"

namespace {

// Partial-sum slab of the surrogate-shape kernels for a batch of B columns.
int64_t wide_slab_elems(const kanode_handle* h, int64_t B) {
    int64_t m = 0;
    for (int l = 0; l < h->n_layers; ++l) {
        const LayerConst& c = h->hlc[l];
        if (h->kind[l] == KIND_WIDE_IN) m = std::max<int64_t>(m, (int64_t)kan::widein_chunks(c) * B * c.O);
        if (h->kind[l] == KIND_WIDE_OUT) m = std::max<int64_t>(m, (int64_t)c.I * (c.G + 1) * B);
    }
    return m;
}

// Chain workspace layout (elements of the dtype), for a batch of B columns:
//   [hidden activations: Σ_{l>=1} I_l·B][grad ping: max_dim·B][grad pong: max_dim·B][wide slab]
//   [surrogate pair: the wide-in layer's chunk partials, chunks·B·H]
struct WsLayout {
    int64_t acts, g0, g1, wslab, pslab, sslab, bslab, pair2, total;   // pair2: offset of the second copy of [pslab, pair2)
};
WsLayout ws_layout(const kanode_handle* h, int64_t B) {
    WsLayout w{};
    int64_t e = 0;
    w.acts = e;
    for (int l = 1; l < h->n_layers; ++l) e += (int64_t)h->hlc[l].I * B;
    w.g0 = e;
    e += (int64_t)h->max_dim * B;
    w.g1 = e;
    e += (int64_t)h->max_dim * B;
    w.wslab = e;
    e += wide_slab_elems(h, B);
    w.pslab = e;
    if (surrogate_pair(h)) e += (int64_t)kan::widein_chunks(h->hlc[0]) * B * h->hlc[0].O;
    // [surrogate pair, two-launch pullback: the wide-out dot products' chunk partials, chunks·H·(G+1)·B]
    w.sslab = e;
    if (surrogate_pair(h)) e += (int64_t)kan::widein_chunks(h->hlc[0]) * h->hlc[1].I * (h->hlc[1].G + 1) * B;
    // [surrogate pair, two-launch pullback: the wide-in layer's basis store, B·I·(G + 2)]
    w.bslab = e;
    if (surrogate_pair(h)) e += kan::pair_basis_elems(h->hlc[0], B);
    // [surrogate pair: the second buffer of the ping-pong pairs pslab .. bslab (fused deferred stages)]
    w.pair2 = e;
    if (surrogate_pair(h)) e += e - w.pslab;
    w.total = e;
    return w;
}

size_t chain_ws_bytes(const kanode_handle* h, int64_t B) { return (size_t)ws_layout(h, B).total * h->esize; }

// the workspace holds `need` bytes (contents not kept): never grown under capture, and only once what reads it has run
kanode_status grow_ws(kanode_handle* h, size_t need, hipStream_t st, const char* capture_msg) {
    if (need <= h->ws.bytes()) return KANODE_OK;
    if (is_capturing(st)) return fail(h, KANODE_ERR_CAPTURE, capture_msg);
    // a deferred surrogate-pair stage reads the old workspace: launch it before the buffer goes away
    if (kanode_status s = flush_pair(h, st); s != KANODE_OK) return s;
    HIP_TRY(h, hipStreamSynchronize(st));
    HIP_TRY(h, h->ws.reserve(need));
    return KANODE_OK;
}

// one region of the deferred reduction slab: [grid][G+1] partials + [grid] error partials, grid <= kSlabBlocks/2
constexpr size_t kDeferRegion = (size_t)(kSlabBlocks / 2) * (kan::kMaxGrid + 2);

}  // namespace

kanode_status ensure_ws(kanode_handle* h, int64_t B, hipStream_t st) {
    return grow_ws(h, h->spec.rhs_kind == KANODE_RHS_CHAIN ? chain_ws_bytes(h, B) : 0, st,
                   "batch exceeds reserved workspace during stream capture; call kanode_reserve");
}
// ... and the Fisher-KPP VJP's λJ when the caller passes none
kanode_status ensure_fk_ws(kanode_handle* h, int64_t B, hipStream_t st) {
    return grow_ws(h, (size_t)(h->spec.nx * B) * h->esize, st, "workspace too small during capture");
}

// stage workspace of at least `need` bytes (the unfused stage paths)
kanode_status ensure_stage_ws(kanode_handle* h, size_t need, hipStream_t st) {
    if (need <= h->stage_ws.bytes()) return KANODE_OK;
    if (is_capturing(st)) return fail(h, KANODE_ERR_CAPTURE, "stage workspace too small during capture");
    if (kanode_status s = flush_pair(h, st); s != KANODE_OK) return s;   // (reads the old stage workspace)
    HIP_TRY(h, hipStreamSynchronize(st));
    HIP_TRY(h, h->stage_ws.reserve(need));
    return KANODE_OK;
}

// The fixed-size reduction slabs of the Fisher-KPP table adjoint (deferred stage reductions and the
// one-launch adjoint step).  kanode_create allocates them for handles that can take that path; this
// covers a handle whose table path was switched on later, and refuses to allocate under capture.
kanode_status ensure_adjoint_slabs(kanode_handle* h, hipStream_t st, bool at_create) {
    if (h->defer_slab.ptr() && h->step_slab.ptr() && h->fin_ctr.ptr()) return KANODE_OK;
    if (!at_create && is_capturing(st))
        return fail(h, KANODE_ERR_CAPTURE, "adjoint reduction slabs would be allocated during capture");
    const size_t defer = kDeferRegion * sizeof(double) * kan::kMaxFinishJobs;
    const size_t step = (size_t)(kSlabBlocks / 2) * (6 * (kan::kMaxGrid + 1) + 1) * sizeof(double);
    if (h->defer_slab.reserve(defer) != hipSuccess || h->step_slab.reserve(step) != hipSuccess)
        return fail(h, KANODE_ERR_ALLOC, "adjoint reduction slabs");
    if (!h->fin_ctr.ptr()) {   // the fused finish's arrival counters: zero here, and back to zero after every step
        if (h->fin_ctr.reserve(2 * sizeof(unsigned)) != hipSuccess ||
            hipMemset(h->fin_ctr.ptr(), 0, 2 * sizeof(unsigned)) != hipSuccess) {
            (void)hipGetLastError();
            h->fin_ctr.reset();
            return fail(h, KANODE_ERR_ALLOC, "adjoint finish counters");
        }
    }
    return KANODE_OK;
}

namespace {

template <typename T>
kan::PairPlan<T>& pair_pending(kanode_handle* h);
template <>
kan::PairPlan<double>& pair_pending<double>(kanode_handle* h) { return h->pend_d; }
template <>
kan::PairPlan<float>& pair_pending<float>(kanode_handle* h) { return h->pend_f; }

}  // namespace

// the deferred surrogate-pair stage's second launch, alone (nothing to fuse it with)
kanode_status flush_pair(kanode_handle* h, hipStream_t st) {
    if (!h->pend_valid) return KANODE_OK;
    h->pend_valid = false;
    const hipError_t e = by_dtype(h, [&](auto t) {
        using T = decltype(t);
        return kan::launch_pair_second<T>(pair_pending<T>(h), nullptr, st);
    });
    if (e != hipSuccess) return fail(h, KANODE_ERR_HIP, std::string("launch_pair_second: ") + hipGetErrorString(e));
    return KANODE_OK;
}

kanode_status vjp_flush(kanode_handle* h, hipStream_t st) {
    if (kanode_status s = flush_pair(h, st); s != KANODE_OK) return s;
    if (h->njobs == 0) return KANODE_OK;
    const int n = h->njobs;
    h->njobs = 0;
    HIP_TRY(h, kan::launch_vjp_finish_jobs(h->jobs, n, fk_moment_len(h), st));
    return KANODE_OK;
}

namespace {

// The wide kernels need the chain workspace's slab (sized by ensure_ws(K)).
template <typename T>
T* wide_slab(kanode_handle* h, int64_t K) {
    return (T*)h->ws.ptr() + ws_layout(h, K).wslab;
}

template <typename T>
kanode_status layer_fwd_t(kanode_handle* h, int l, const T* p_full, const T* x, T* y, int64_t K, hipStream_t st) {
    const LayerConst& hl = h->hlc[l];
    switch (h->kind[l]) {
    case KIND_COL:
        HIP_TRY(h, kan::launch_kd_fwd_col<T>(hl, h->dlc() + l, p_full, x, y, K, st));
        return KANODE_OK;
    case KIND_WIDE_IN:
        HIP_TRY(h, kan::launch_kd_fwd_widein<T>(hl, h->dlc() + l, p_full, x, y, wide_slab<T>(h, K), K, st));
        return KANODE_OK;
    case KIND_WIDE_OUT:
        HIP_TRY(h, kan::launch_kd_fwd_wideout<T>(hl, h->dlc() + l, p_full, x, y, K, st));
        return KANODE_OK;
    }
    return fail(h, KANODE_ERR_UNSUPPORTED, "layer kind");
}

template <typename T>
kanode_status layer_vjp_t(kanode_handle* h, int l, const T* p_full, const T* x, const T* yb, T* xb, T* pbar_full,
                          int64_t K, hipStream_t st) {
    const LayerConst& hl = h->hlc[l];
    switch (h->kind[l]) {
    case KIND_COL:
        HIP_TRY(h, kan::launch_kd_vjp_col<T>(hl, h->dlc() + l, p_full, x, yb, xb, pbar_full, (T*)h->slab.ptr(), kSlabBlocks,
                                             K, st));
        return KANODE_OK;
    case KIND_WIDE_IN:
        HIP_TRY(h, kan::launch_kd_vjp_widein<T>(hl, h->dlc() + l, p_full, x, yb, xb, pbar_full, K, st));
        return KANODE_OK;
    case KIND_WIDE_OUT:
        HIP_TRY(h, kan::launch_kd_vjp_wideout<T>(hl, h->dlc() + l, p_full, x, yb, xb, pbar_full, wide_slab<T>(h, K), K,
                                                 st));
        return KANODE_OK;
    }
    return fail(h, KANODE_ERR_UNSUPPORTED, "layer kind");
}

template <typename T>
kanode_status rhs_t(kanode_handle* h, const T* p, const T* u, T* du, int64_t B, hipStream_t st) {
    if (h->spec.rhs_kind == KANODE_RHS_POINTWISE_PERIODIC_LAPLACIAN) {
        const FkLap lap = fk_lap(h);
        const T cd = (T)lap.cd, co = (T)lap.co;
        if constexpr (std::is_same<T, double>::value) {
            if (h->opt.pp_on) {
                HIP_TRY(h, kan::launch_fk_rhs_pp(h->hpc, h->hlc[0], h->dlc(), h->dpc(), p, h->dtable(), cd, co, (int)h->spec.nx, u, du,
                                                 B, st, table_build(h, h->built_phi), h->opt.grid_rhs,
                                                 &h->fk_launch));
                served(h, KANODE_EVAL_FK_TABLE);
                return KANODE_OK;
            }
        }
        HIP_TRY(h, kan::launch_fk_rhs<T>(h->hlc[0], h->dlc(), p, cd, co, (int)h->spec.nx, u, du, B, st));
        served(h, KANODE_EVAL_FK_POINT);
        return KANODE_OK;
    }
    // (only here: a single column layer takes its own layer kernel, not the one-launch chain kernel)
    if (h->n_layers > 1 && all_col(h)) {
        bool done = false;
        const hipError_t e = kan::launch_kd_chain_col<T>(h->hlc, h->n_layers, h->dlc(), p, h->P, u, du, B, st);
        if (kanode_status s = launched_or_error(h, e, "launch_kd_chain_col", done, KANODE_EVAL_CHAIN_KERNEL);
            s != KANODE_OK || done)
            return s;
    }
    kanode_status s = ensure_ws(h, B, st);
    if (s != KANODE_OK) return s;
    T* ws = (T*)h->ws.ptr();
    const WsLayout wl = ws_layout(h, B);
    if (surrogate_pair(h)) {   // two launches: wide-in partials -> wide-out summing them itself
        T* ps = ws + wl.pslab;
        HIP_TRY(h, kan::launch_kd_fwd_widein<T>(h->hlc[0], h->dlc(), p, u, (T*)nullptr, ps, B, st));
        HIP_TRY(h, kan::launch_kd_fwd_wideout<T>(h->hlc[1], h->dlc() + 1, p, (const T*)nullptr, du, B, st, ps,
                                                  kan::widein_chunks(h->hlc[0])));
        served(h, KANODE_EVAL_PAIR);
        return KANODE_OK;
    }
    served(h, KANODE_EVAL_PER_LAYER);
    const T* cur = u;
    for (int l = 0; l < h->n_layers; ++l) {
        T* out = (l == h->n_layers - 1) ? du : ws + ((l % 2) ? wl.g1 : wl.g0);
        s = layer_fwd_t<T>(h, l, p, cur, out, B, st);
        if (s != KANODE_OK) return s;
        cur = out;
    }
    return KANODE_OK;
}

template <typename T>
kanode_status vjp_t(kanode_handle* h, const T* p, const T* u, const T* lam, T* lamJ, T* dp, int64_t B,
                    hipStream_t st) {
    if (h->spec.rhs_kind == KANODE_RHS_POINTWISE_PERIODIC_LAPLACIAN) {
        const FkLap lap = fk_lap(h);
        const T cd = (T)lap.cd, co = (T)lap.co;
        // lam_J is needed for the kernel's store; use workspace when the caller passes NULL
        T* out = lamJ;
        if (!out) {
            if (kanode_status s = ensure_fk_ws(h, B, st); s != KANODE_OK) return s;
            out = (T*)h->ws.ptr();
        }
        if constexpr (std::is_same<T, double>::value) {
            if (h->opt.pp_on && kan::fk_vjp_pp_supported(h->hlc[0], (int)h->spec.nx)) {
                HIP_TRY(h, kan::launch_fk_vjp_pp(h->hpc, h->hlc[0], h->dlc(), h->dpc(), p, h->dtable(), cd, co,
                                                 (int)h->spec.nx, u, lam, out, dp, (double*)h->slab.ptr(), kSlabBlocks, B,
                                                 st, table_build(h, h->built_vjp), h->opt.grid_vjp, &h->fk_launch));
                served(h, KANODE_EVAL_FK_TABLE);
                return KANODE_OK;
            }
        }
        HIP_TRY(h, kan::launch_fk_vjp<T>(h->hlc[0], h->dlc(), p, cd, co, (int)h->spec.nx, u, lam, out, dp, (T*)h->slab.ptr(),
                                         kSlabBlocks, B, st));
        served(h, KANODE_EVAL_FK_POINT);
        return KANODE_OK;
    }
    if (lamJ && h->n_in == h->n_out && all_col(h)) {
        const kan::StageArgs<T> none{};
        bool done = false;
        const hipError_t e = kan::launch_kd_chain_vjp_stage<T>(h->hlc, h->n_layers, h->dlc(), p, h->P, u, none, lam,
                                                               none, nullptr, lamJ, dp, false, nullptr, h->slab.ptr(),
                                                               h->slab.bytes(), B, st);
        if (kanode_status s = launched_or_error(h, e, "launch_kd_chain_vjp_stage", done, KANODE_EVAL_CHAIN_KERNEL);
            s != KANODE_OK || done)
            return s;
    }
    kanode_status s = ensure_ws(h, B, st);
    if (s != KANODE_OK) return s;
    T* ws = (T*)h->ws.ptr();
    const WsLayout wl = ws_layout(h, B);
    if (surrogate_pair(h)) {
        served(h, KANODE_EVAL_PAIR);
        T* ps = ws + wl.pslab;
        T* hbar = ws + wl.g0;
        const int nb = kan::widein_chunks(h->hlc[0]);
        if (lamJ && h->opt.pair_vjp) {
            // two launches (launch_kd_vjp_pair): the wide-in forward blocks also form the wide-out dot
            // products' chunk partials; the wide-out parameter cotangents beside the wide-in pullback
            // (x̄ of the hidden layer formed per block)
            bool done = false;
            const hipError_t e = kan::launch_kd_vjp_pair<T>(h->hlc[0], h->hlc[1], h->dlc(), p, u, nullptr, lam, u, ps,
                                                            ws + wl.sslab, lamJ, dp, B, st, false, nullptr, 0,
                                                            nullptr, ws + wl.bslab);
            if ((s = launched_or_error(h, e, "launch_kd_vjp_pair", done)) != KANODE_OK || done) return s;
        }
        // four launches: wide-in partials; the wide-out pullback's dot products and parameter
        // cotangents in one launch; its input cotangent; the wide-in pullback
        HIP_TRY(h, kan::launch_kd_fwd_widein<T>(h->hlc[0], h->dlc(), p, u, (T*)nullptr, ps, B, st));
        HIP_TRY(h, kan::launch_kd_vjp_wideout<T>(h->hlc[1], h->dlc() + 1, p, (const T*)nullptr, lam, hbar, dp,
                                                  ws + wl.wslab, B, st, ps, nb));
        if (lamJ || dp) HIP_TRY(h, kan::launch_kd_vjp_widein<T>(h->hlc[0], h->dlc(), p, u, hbar, lamJ, dp, B, st));
        return KANODE_OK;
    }
    // forward recompute, keeping every hidden layer's input
    served(h, KANODE_EVAL_PER_LAYER);
    const T* acts[KANODE_MAX_LAYERS];
    acts[0] = u;
    T* wp = ws + wl.acts;
    for (int l = 1; l < h->n_layers; ++l) {
        T* out = wp;
        wp += (int64_t)h->hlc[l].I * B;
        s = layer_fwd_t<T>(h, l - 1, p, acts[l - 1], out, B, st);
        if (s != KANODE_OK) return s;
        acts[l] = out;
    }
    T* g0 = ws + wl.g0;
    T* g1 = ws + wl.g1;
    const T* g = lam;
    for (int l = h->n_layers - 1; l >= 0; --l) {
        T* out = (l == 0) ? lamJ : ((l % 2) ? g0 : g1);
        if (l == 0 && !out) out = (g == g0) ? g1 : g0;   // caller skipped lam_J
        s = layer_vjp_t<T>(h, l, p, acts[l], g, out, dp, B, st);
        if (s != KANODE_OK) return s;
        g = out;
    }
    return KANODE_OK;
}

// a kanode_stage as the kernels take it: the earlier stage vectors, their coefficients and the error weights
template <typename T>
kanode_status stage_args(kanode_handle* h, const kanode_stage* sg, kan::StageArgs<T>& sa) {
    if (sg->n_prev < 0 || sg->n_prev > KANODE_MAX_STAGES)
        return fail(h, KANODE_ERR_INVALID_ARG, "n_prev must be in [0, KANODE_MAX_STAGES]");
    sa = kan::StageArgs<T>{};
    sa.nk = sg->n_prev;
    for (int j = 0; j < sg->n_prev; ++j) {
        if (!sg->k[j]) return fail(h, KANODE_ERR_INVALID_ARG, "null stage vector k[" + std::to_string(j) + "]");
        sa.k[j] = (const T*)sg->k[j];
        sa.c[j] = sg->c[j];
    }
    for (int j = 0; j <= sg->n_prev; ++j) sa.ec[j] = sg->want_error ? sg->ec[j] : 0.0;
    sa.abstol = sg->abstol;
    sa.reltol = sg->reltol;
    return KANODE_OK;
}

template <typename T>
kanode_status stage_t(kanode_handle* h, const T* p, const T* u, const kanode_stage* sg, T* du, int64_t B,
                      hipStream_t st, const double* cscale = nullptr, const int32_t* skip = nullptr) {
    // (the n_prev range is refused before the two checks below, the null stage vectors after them)
    if (sg->n_prev < 0 || sg->n_prev > KANODE_MAX_STAGES)
        return fail(h, KANODE_ERR_INVALID_ARG, "n_prev must be in [0, KANODE_MAX_STAGES]");
    if (h->n_in != h->n_out) return fail(h, KANODE_ERR_INVALID_ARG, "stage needs an RHS with N_in == N_out");
    if (sg->want_error && !sg->error_sumsq) return fail(h, KANODE_ERR_INVALID_ARG, "want_error needs error_sumsq");
    kan::StageArgs<T> sa;
    if (kanode_status s = stage_args<T>(h, sg, sa); s != KANODE_OK) return s;
    sa.cscale = cscale;
    sa.skip = skip;
    double* err_out = sg->want_error ? (double*)sg->error_sumsq : nullptr;
    if constexpr (std::is_same<T, double>::value) {
        if (fk_table_path(h) && kan::fk_stage_pp_supported(h->hpc, (int)h->spec.nx)) {
            const auto [cd, co] = fk_lap(h);
            HIP_TRY(h, kan::launch_fk_stage_pp(h->hpc, h->hlc[0], h->dlc(), h->dpc(), p, h->dtable(), cd, co,
                                               (int)h->spec.nx, u, sa, (double*)sg->y_out, (double*)h->slab.ptr(),
                                               kSlabBlocks, err_out, du, B, st, table_build(h, h->built_phi),
                                               h->opt.grid_rhs, &h->fk_launch));
            served(h, KANODE_EVAL_FK_TABLE);
            return KANODE_OK;
        }
    }
    if (h->spec.rhs_kind == KANODE_RHS_CHAIN && all_col(h)) {
        // a small chain: stage input, RHS and error partials in one kernel (kd_chain_col_kernel)
        bool done = false;
        const hipError_t e = kan::launch_kd_chain_col<T>(h->hlc, h->n_layers, h->dlc(), p, h->P, u, du, B, st, &sa,
                                                         (T*)sg->y_out, (double*)h->slab.ptr(), kSlabBlocks, err_out);
        if (kanode_status s = launched_or_error(h, e, "launch_kd_chain_col", done, KANODE_EVAL_CHAIN_KERNEL);
            s != KANODE_OK || done)
            return s;
    }
    const int64_t n = h->n_in * B;
    if (h->spec.rhs_kind == KANODE_RHS_CHAIN && surrogate_pair(h) && !skip) {
        // surrogate pair: the wide-in forward forms y itself (kd_fwd_widein_co_kernel stage input)
        kanode_status s = ensure_ws(h, B, st);
        if (s != KANODE_OK) return s;
        T* y = (T*)sg->y_out;
        if (!y && err_out) {
            if ((s = ensure_stage_ws(h, (size_t)n * sizeof(T), st)) != KANODE_OK) return s;
            y = (T*)h->stage_ws.ptr();
        }
        T* ps = (T*)h->ws.ptr() + ws_layout(h, B).pslab;
        kan::WideStageIn<T> si{};
        si.su = sa;
        si.y_out = y;
        HIP_TRY(h, kan::launch_kd_fwd_widein<T>(h->hlc[0], h->dlc(), p, u, (T*)nullptr, ps, B, st, &si));
        HIP_TRY(h, kan::launch_kd_fwd_wideout<T>(h->hlc[1], h->dlc() + 1, p, (const T*)nullptr, du, B, st, ps,
                                                  kan::widein_chunks(h->hlc[0])));
        if (err_out) HIP_TRY(h, kan::launch_stage_error<T>(u, y, du, sa, (double*)h->slab.ptr(), kSlabBlocks, err_out, n, st));
        served(h, KANODE_EVAL_PAIR);
        return KANODE_OK;
    }
    // unfused: y materialised (into y_out or the handle's stage workspace), RHS, error pass
    T* y = (T*)sg->y_out;
    if (!y) {
        kanode_status s = ensure_stage_ws(h, (size_t)n * sizeof(T), st);
        if (s != KANODE_OK) return s;
        y = (T*)h->stage_ws.ptr();
    }
    HIP_TRY(h, kan::launch_stage_lincomb<T>(u, sa, y, n, st));
    kanode_status s = rhs_t<T>(h, p, y, du, B, st);
    if (s != KANODE_OK) return s;
    if (err_out) HIP_TRY(h, kan::launch_stage_error<T>(u, y, du, sa, (double*)h->slab.ptr(), kSlabBlocks, err_out, n, st));
    return KANODE_OK;
}

template <typename T>
kanode_status vjp_stage_t(kanode_handle* h, const T* p, const T* u, const kanode_stage* state, const T* lam,
                          const kanode_stage* adj, T* lamJ, T* dp, int64_t B, hipStream_t st, bool dp_assign = false,
                          const double* su_scale = nullptr, const double* sl_scale = nullptr, bool defer = false) {
    if (h->n_in != h->n_out) return fail(h, KANODE_ERR_INVALID_ARG, "adjoint stage needs an RHS with N_in == N_out");
    if (adj->want_error && !adj->error_sumsq) return fail(h, KANODE_ERR_INVALID_ARG, "want_error needs error_sumsq");
    kan::StageArgs<T> su, sl;
    kanode_status s = stage_args<T>(h, state, su);
    if (s != KANODE_OK) return s;
    s = stage_args<T>(h, adj, sl);
    if (s != KANODE_OK) return s;
    su.cscale = su_scale;
    sl.cscale = sl_scale;
    const int64_t n = h->n_in * B;
    double* err_out = adj->want_error ? (double*)adj->error_sumsq : nullptr;
    if constexpr (std::is_same<T, double>::value) {
        // Fisher-KPP table path: the whole adjoint stage in one streaming kernel + one reduction
        if (fk_table_path(h) && lamJ && kan::fk_vjp_pp_supported(h->hlc[0], (int)h->spec.nx)) {
            served(h, KANODE_EVAL_FK_TABLE);
            const auto [cd, co] = fk_lap(h);
            if (defer && (dp || err_out)) {
                if (h->njobs == kan::kMaxFinishJobs && (s = vjp_flush(h, st)) != KANODE_OK) return s;
                if ((s = ensure_adjoint_slabs(h, st)) != KANODE_OK) return s;
                double* region = (double*)h->defer_slab.ptr() + (size_t)h->njobs * kDeferRegion;
                int grid = 0;
                HIP_TRY(h, kan::launch_fk_vjp_stage_pp(h->hpc, h->hlc[0], h->dlc(), h->dpc(), p, h->dtable(), cd, co,
                                                       (int)h->spec.nx, u, su, lam, sl, (double*)adj->y_out, lamJ,
                                                       dp, dp_assign, err_out, region, kSlabBlocks, B, st,
                                                       table_build(h, h->built_vjp), &grid, h->opt.grid_vjp,
                                                       &h->fk_launch));
                kan::FinishJob& jb = h->jobs.j[h->njobs++];
                jb.slab = region;
                jb.err_slab = region + (int64_t)grid * (h->hlc[0].G + 1);   // (the region's row stride, not fk_moment_len)
                jb.dp = dp;
                jb.err_out = err_out;
                jb.nblk = grid;
                jb.assign = dp_assign ? 1 : 0;
                return KANODE_OK;
            }
            HIP_TRY(h, kan::launch_fk_vjp_stage_pp(h->hpc, h->hlc[0], h->dlc(), h->dpc(), p, h->dtable(), cd, co,
                                                   (int)h->spec.nx, u, su, lam, sl, (double*)adj->y_out, lamJ, dp,
                                                   dp_assign, err_out, (double*)h->slab.ptr(), kSlabBlocks, B, st,
                                                   table_build(h, h->built_vjp), nullptr, h->opt.grid_vjp,
                                                   &h->fk_launch));
            return KANODE_OK;
        }
    }
    if (h->spec.rhs_kind == KANODE_RHS_CHAIN && lamJ && all_col(h)) {
        // a small chain: the whole adjoint stage in one kernel (kd_chain_vjp_stage_kernel) + one reduction
        bool done = false;
        const hipError_t e = kan::launch_kd_chain_vjp_stage<T>(h->hlc, h->n_layers, h->dlc(), p, h->P, u, su, lam, sl,
                                                               (T*)adj->y_out, lamJ, dp, dp_assign, err_out,
                                                               h->slab.ptr(), h->slab.bytes(), B, st);
        if ((s = launched_or_error(h, e, "launch_kd_chain_vjp_stage", done, KANODE_EVAL_CHAIN_KERNEL)) != KANODE_OK || done)
            return s;
    }
    if (h->spec.rhs_kind == KANODE_RHS_CHAIN && surrogate_pair(h) && lamJ) {
        served(h, KANODE_EVAL_PAIR);
        // surrogate pair: y and λs formed by the wide-in forward (no combination launches), the
        // parameter cotangents written with = when dp_assign (no memset): four launches per stage.
        // Deferred stages (the integrator's, `defer`) run lazily: a stage's second launch waits for the next
        // stage and both run as one (launch_pair_second with next), alternating the ping-pong buffers.
        const bool lazy = defer && h->opt.pair_vjp && h->opt.pair_fuse;
        if (!lazy || chain_ws_bytes(h, B) > h->ws.bytes() || 4 * (size_t)n * sizeof(T) > h->stage_ws.bytes())
            if ((s = flush_pair(h, st)) != KANODE_OK) return s;   // (and before any buffer is reallocated)
        if ((s = ensure_ws(h, B, st)) != KANODE_OK) return s;
        if ((s = ensure_stage_ws(h, 4 * (size_t)n * sizeof(T), st)) != KANODE_OK) return s;
        const int par = lazy ? h->pair_par : 0;
        const WsLayout wl = ws_layout(h, B);
        T* ws = (T*)h->ws.ptr();
        const int64_t pp = par ? wl.pair2 - wl.pslab : 0;   // the ping-pong pairs' second buffer
        T* y = (T*)h->stage_ws.ptr() + (size_t)par * 2 * n;
        T* ls = adj->y_out ? (T*)adj->y_out : y + n;
        T* ps = ws + wl.pslab + pp;
        T* hbar = ws + wl.g0;
        const int nb = kan::widein_chunks(h->hlc[0]);
        kan::WideStageIn<T> si{};
        si.su = su;
        si.y_out = y;
        si.lam = lam;
        si.sl = sl;
        si.ls_out = ls;
        // the two launches' plan (see vjp_t); with the integrator's mapped buffer the host sums the λ error's
        // partials, so the plan loses its final launch
        auto plan = [&](kan::PairPlan<T>& pl) {
            const bool host_parts = err_out && h->err_parts && h->err_nparts;
            const hipError_t e = kan::plan_kd_vjp_pair<T>(
                h->hlc[0], h->hlc[1], h->dlc(), p, u, &si, lam, y, ps, ws + wl.sslab + pp, lamJ, dp, B, dp_assign,
                host_parts ? h->err_parts : (double*)h->slab.ptr(), kSlabBlocks, err_out, ws + wl.bslab + pp, &pl);
            if (e == hipSuccess && host_parts && pl.err_out) {
                *h->err_nparts = pl.err_rows;
                pl.err_out = nullptr;
            }
            return e;
        };
        hipError_t e = hipErrorNotSupported;
        bool err_done = false;
        if (h->opt.pair_vjp) {   // (lazy implies it)
            kan::PairPlan<T> pl;
            e = plan(pl);
            if (e != hipSuccess && e != hipErrorNotSupported)
                return fail(h, KANODE_ERR_HIP, std::string("plan_kd_vjp_pair: ") + hipGetErrorString(e));
            if (e == hipSuccess && lazy) {
                kan::PairPlan<T>& pend = pair_pending<T>(h);
                if (h->pend_valid) e = kan::launch_pair_second<T>(pend, &pl, st);
                else e = kan::launch_pair_first<T>(pl, st);
                if (e != hipSuccess)
                    return fail(h, KANODE_ERR_HIP, std::string("pair stage: ") + hipGetErrorString(e));
                pend = pl;
                h->pend_valid = true;
                h->pair_par ^= 1;
                return KANODE_OK;
            }
            if (e == hipSuccess) {   // two launches, plus the λ error's final sum
                if ((e = kan::launch_pair_first<T>(pl, st)) == hipSuccess) e = kan::launch_pair_second<T>(pl, nullptr, st);
                if (e != hipSuccess) return fail(h, KANODE_ERR_HIP, std::string("pair stage: ") + hipGetErrorString(e));
                err_done = err_out != nullptr;
            } else if (lazy && (s = flush_pair(h, st)) != KANODE_OK) {
                return s;
            }
        }
        if (e != hipSuccess) {
            HIP_TRY(h, kan::launch_kd_fwd_widein<T>(h->hlc[0], h->dlc(), p, u, (T*)nullptr, ps, B, st, &si));
            HIP_TRY(h, kan::launch_kd_vjp_wideout<T>(h->hlc[1], h->dlc() + 1, p, (const T*)nullptr, ls, hbar, dp,
                                                      ws + wl.wslab, B, st, ps, nb, dp_assign));
            HIP_TRY(h, kan::launch_kd_vjp_widein<T>(h->hlc[0], h->dlc(), p, y, hbar, lamJ, dp, B, st, dp_assign));
        }
        if (err_out && !err_done)
            HIP_TRY(h, kan::launch_stage_error<T>(lam, ls, lamJ, sl, (double*)h->slab.ptr(), kSlabBlocks, err_out, n, st));
        return KANODE_OK;
    }
    if (dp && dp_assign) HIP_TRY(h, hipMemsetAsync(dp, 0, (size_t)h->P * sizeof(T), st));
    if ((s = ensure_stage_ws(h, 2 * (size_t)n * sizeof(T), st)) != KANODE_OK) return s;
    T* y = su.nk ? (T*)h->stage_ws.ptr() : (T*)u;
    T* ls = adj->y_out ? (T*)adj->y_out : (sl.nk ? (T*)h->stage_ws.ptr() + n : (T*)lam);
    if (su.nk) HIP_TRY(h, kan::launch_stage_lincomb<T>(u, su, y, n, st));
    if (sl.nk || adj->y_out) HIP_TRY(h, kan::launch_stage_lincomb<T>(lam, sl, ls, n, st));
    if ((s = vjp_t<T>(h, p, y, ls, lamJ, dp, B, st)) != KANODE_OK) return s;
    if (err_out) HIP_TRY(h, kan::launch_stage_error<T>(lam, ls, lamJ, sl, (double*)h->slab.ptr(), kSlabBlocks, err_out, n, st));
    return KANODE_OK;
}

// one layer at a stage input (kanode_layer_forward_stage): y = x + Σ c·k (and λs = lam + Σ c·k) formed by the
// wide-in forward's blocks themselves (kd_fwd_widein_stage_kernel, the fma order of stage_lincomb_kernel);
// any other layer kind gets the combinations as their own launches first
template <typename T>
kanode_status layer_fwd_stage_t(kanode_handle* h, int l, const T* p_full, const T* x, const kanode_stage* sx,
                                const T* lam, const kanode_stage* sl, T* out, int64_t K, hipStream_t st) {
    kan::StageArgs<T> su{}, sla{};
    kanode_status s = stage_args<T>(h, sx, su);
    if (s != KANODE_OK) return s;
    if (lam && (s = stage_args<T>(h, sl, sla)) != KANODE_OK) return s;
    const LayerConst& hl = h->hlc[l];
    const int64_t n = (int64_t)hl.I * K;
    if (h->kind[l] == KIND_WIDE_IN) {
        kan::WideStageIn<T> si{};
        si.su = su;
        si.y_out = (T*)sx->y_out;
        si.lam = lam;
        si.sl = sla;
        si.ls_out = lam ? (T*)sl->y_out : nullptr;
        HIP_TRY(h, kan::launch_kd_fwd_widein<T>(hl, h->dlc() + l, p_full, x, out, wide_slab<T>(h, K), K, st, &si));
        return KANODE_OK;
    }
    T* y = (T*)sx->y_out;
    if (!y) {
        if ((s = ensure_stage_ws(h, (size_t)n * sizeof(T), st)) != KANODE_OK) return s;
        y = (T*)h->stage_ws.ptr();
    }
    HIP_TRY(h, kan::launch_stage_lincomb<T>(x, su, y, n, st));
    if (lam) HIP_TRY(h, kan::launch_stage_lincomb<T>(lam, sla, (T*)sl->y_out, n, st));
    return layer_fwd_t<T>(h, l, p_full, y, out, K, st);
}

}  // namespace

// The public entry points check in this order: handle, (stage / layer), negative batch, zero batch -> OK, null
// pointers; each keeps its own null-pointer text.
extern "C" {

kanode_status kanode_rhs(kanode_handle* h, const void* p, const void* u, void* du, int64_t batch, void* stream) {
    kanode_status s = check_handle(h);
    if (s != KANODE_OK) return s;
    if (batch < 0) return fail(h, KANODE_ERR_INVALID_ARG, "batch < 0");
    if (batch == 0) return KANODE_OK;
    if (!p || !u || !du) return fail(h, KANODE_ERR_INVALID_ARG, "null pointer");
    return by_dtype(h, [&](auto t) {
        using T = decltype(t);
        return rhs_t<T>(h, (const T*)p, (const T*)u, (T*)du, batch, (hipStream_t)stream);
    });
}

kanode_status kanode_rhs_stage(kanode_handle* h, const void* p, const void* u, const kanode_stage* stage, void* du,
                               int64_t batch, void* stream) {
    kanode_status s = check_handle(h);
    if (s != KANODE_OK) return s;
    if (!stage) return fail(h, KANODE_ERR_INVALID_ARG, "null stage");
    if (batch < 0) return fail(h, KANODE_ERR_INVALID_ARG, "batch < 0");
    if (batch == 0) return KANODE_OK;
    if (!p || !u || !du) return fail(h, KANODE_ERR_INVALID_ARG, "null p/u/du");
    return by_dtype(h, [&](auto t) {
        using T = decltype(t);
        return stage_t<T>(h, (const T*)p, (const T*)u, stage, (T*)du, batch, (hipStream_t)stream);
    });
}

kanode_status kanode_vjp_stage(kanode_handle* h, const void* p, const void* u, const kanode_stage* state,
                               const void* lam, const kanode_stage* adj, void* lamJ, void* dp, int64_t batch,
                               void* stream) {
    kanode_status s = check_handle(h);
    if (s != KANODE_OK) return s;
    if (!state || !adj) return fail(h, KANODE_ERR_INVALID_ARG, "null stage");
    if (batch < 0) return fail(h, KANODE_ERR_INVALID_ARG, "batch < 0");
    if (batch == 0) return KANODE_OK;
    if (!p || !u || !lam || !lamJ) return fail(h, KANODE_ERR_INVALID_ARG, "null p/u/lam/lamJ");
    return by_dtype(h, [&](auto t) {
        using T = decltype(t);
        return vjp_stage_t<T>(h, (const T*)p, (const T*)u, state, (const T*)lam, adj, (T*)lamJ, (T*)dp, batch,
                              (hipStream_t)stream);
    });
}

kanode_status kanode_vjp(kanode_handle* h, const void* p, const void* u, const void* lam, void* lam_J, void* dp,
                         int64_t batch, void* stream) {
    kanode_status s = check_handle(h);
    if (s != KANODE_OK) return s;
    if (batch < 0) return fail(h, KANODE_ERR_INVALID_ARG, "batch < 0");
    if (batch == 0) return KANODE_OK;
    if (!p || !u || !lam) return fail(h, KANODE_ERR_INVALID_ARG, "null pointer");
    return by_dtype(h, [&](auto t) {
        using T = decltype(t);
        return vjp_t<T>(h, (const T*)p, (const T*)u, (const T*)lam, (T*)lam_J, (T*)dp, batch, (hipStream_t)stream);
    });
}

kanode_status kanode_layer_forward(kanode_handle* h, int32_t layer, const void* p_layer, const void* x, void* y,
                                   int64_t K, void* stream) {
    kanode_status s = check_handle(h);
    if (s != KANODE_OK) return s;
    if (layer < 0 || layer >= h->n_layers) return fail(h, KANODE_ERR_INVALID_ARG, "layer out of range");
    if (K < 0) return fail(h, KANODE_ERR_INVALID_ARG, "K < 0");
    if (K == 0) return KANODE_OK;
    if (!p_layer || !x || !y) return fail(h, KANODE_ERR_INVALID_ARG, "null pointer");
    // kernels index p_full + p_off: shift the caller's layer slice back
    const int64_t off = h->hlc[layer].p_off;
    hipStream_t st = (hipStream_t)stream;
    if ((s = ensure_ws(h, K, st)) != KANODE_OK) return s;
    served(h, KANODE_EVAL_PER_LAYER);
    return by_dtype(h, [&](auto t) {
        using T = decltype(t);
        return layer_fwd_t<T>(h, layer, (const T*)p_layer - off, (const T*)x, (T*)y, K, st);
    });
}

kanode_status kanode_layer_forward_stage(kanode_handle* h, int32_t layer, const void* p_layer, const void* x,
                                         const kanode_stage* sx, const void* lam, const kanode_stage* sl, void* out,
                                         int64_t K, void* stream) {
    kanode_status s = check_handle(h);
    if (s != KANODE_OK) return s;
    if (layer < 0 || layer >= h->n_layers) return fail(h, KANODE_ERR_INVALID_ARG, "layer out of range");
    if (K < 0) return fail(h, KANODE_ERR_INVALID_ARG, "K < 0");
    if (K == 0) return KANODE_OK;
    if (!p_layer || !x || !sx || !out) return fail(h, KANODE_ERR_INVALID_ARG, "null pointer");
    if (lam && (!sl || !sl->y_out)) return fail(h, KANODE_ERR_INVALID_ARG, "lam needs sl with y_out (the λs output)");
    const int64_t off = h->hlc[layer].p_off;
    hipStream_t st = (hipStream_t)stream;
    if ((s = ensure_ws(h, K, st)) != KANODE_OK) return s;
    served(h, KANODE_EVAL_PER_LAYER);
    return by_dtype(h, [&](auto t) {
        using T = decltype(t);
        return layer_fwd_stage_t<T>(h, layer, (const T*)p_layer - off, (const T*)x, sx, (const T*)lam, sl, (T*)out, K, st);
    });
}

kanode_status kanode_layer_vjp(kanode_handle* h, int32_t layer, const void* p_layer, const void* x, const void* ybar,
                               void* xbar, void* pbar_layer, int64_t K, void* stream) {
    kanode_status s = check_handle(h);
    if (s != KANODE_OK) return s;
    if (layer < 0 || layer >= h->n_layers) return fail(h, KANODE_ERR_INVALID_ARG, "layer out of range");
    if (K < 0) return fail(h, KANODE_ERR_INVALID_ARG, "K < 0");
    if (K == 0) return KANODE_OK;
    if (!p_layer || !x || !ybar || !xbar) return fail(h, KANODE_ERR_INVALID_ARG, "null pointer (xbar is required)");
    const int64_t off = h->hlc[layer].p_off;
    hipStream_t st = (hipStream_t)stream;
    if ((s = ensure_ws(h, K, st)) != KANODE_OK) return s;
    served(h, KANODE_EVAL_PER_LAYER);
    return by_dtype(h, [&](auto t) {
        using T = decltype(t);
        return layer_vjp_t<T>(h, layer, (const T*)p_layer - off, (const T*)x, (const T*)ybar, (T*)xbar,
                              pbar_layer ? (T*)pbar_layer - off : nullptr, K, st);
    });
}

kanode_status kanode_edge_activations(kanode_handle* h, int32_t layer, const void* p_layer, const void* x, void* act,
                                      int64_t K, void* stream) {
    kanode_status s = check_handle(h);
    if (s != KANODE_OK) return s;
    if (layer < 0 || layer >= h->n_layers) return fail(h, KANODE_ERR_INVALID_ARG, "layer out of range");
    if (K < 0) return fail(h, KANODE_ERR_INVALID_ARG, "K < 0");
    if (K == 0) return KANODE_OK;
    if (!p_layer || !x || !act) return fail(h, KANODE_ERR_INVALID_ARG, "null pointer");
    const int64_t off = h->hlc[layer].p_off;
    hipStream_t st = (hipStream_t)stream;
    if (h->hlc[layer].O > 64) return fail(h, KANODE_ERR_UNSUPPORTED, "edge activations need out_dims <= 64");
    return by_dtype(h, [&](auto t) {
        using T = decltype(t);
        HIP_TRY(h, kan::launch_kd_edge_act<T>(h->hlc[layer], h->dlc() + layer, (const T*)p_layer - off, (const T*)x,
                                              (T*)act, K, st));
        return KANODE_OK;
    });
}

kanode_status kanode_edge_scores(kanode_handle* h, int32_t layer, const void* p_layer, const void* x, void* scores,
                                 int64_t K, void* stream) {
    kanode_status s = check_handle(h);
    if (s != KANODE_OK) return s;
    if (layer < 0 || layer >= h->n_layers) return fail(h, KANODE_ERR_INVALID_ARG, "layer out of range");
    // (unlike its siblings, K == 0 is refused too)
    if (K <= 0) return fail(h, KANODE_ERR_INVALID_ARG, "kanode_edge_scores: K <= 0 (a maximum over no samples)");
    if (!p_layer || !x || !scores) return fail(h, KANODE_ERR_INVALID_ARG, "null pointer");
    const int64_t off = h->hlc[layer].p_off;
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(h, [&](auto t) {
        using T = decltype(t);
        HIP_TRY(h, kan::launch_kd_edge_scores<T>(h->hlc[layer], h->dlc() + layer, (const T*)p_layer - off, (const T*)x,
                                                 (T*)scores, (T*)h->slab.ptr(), h->slab.bytes(), K, st));
        return KANODE_OK;
    });
}

}  // extern "C"

// ---- the integrator's twins of the entry points above (kanode_internal.hpp) ----
kanode_status kanode_internal_rhs_stage(kanode_handle* h, const void* p, const void* u, const kanode_stage* sg,
                                        void* du, int64_t batch, void* stream, const double* cscale,
                                        const int32_t* skip) {
    kanode_status s = check_handle(h);
    if (s != KANODE_OK) return s;
    if (!p || !u || !du || !sg || batch < 1) return fail(h, KANODE_ERR_INVALID_ARG, "null argument or batch < 1");
    return by_dtype(h, [&](auto t) {
        using T = decltype(t);
        return stage_t<T>(h, (const T*)p, (const T*)u, sg, (T*)du, batch, (hipStream_t)stream, cscale, skip);
    });
}

kanode_status kanode_internal_vjp_stage(kanode_handle* h, const void* p, const void* u, const kanode_stage* state,
                                        const void* lam, const kanode_stage* adj, void* lamJ, void* dp, bool dp_assign,
                                        int64_t batch, void* stream, const double* su_scale, const double* sl_scale,
                                        bool defer) {
    kanode_status s = check_handle(h);
    if (s != KANODE_OK) return s;
    if (!p || !u || !lam || !state || !adj || batch < 1) return fail(h, KANODE_ERR_INVALID_ARG, "null argument or batch < 1");
    return by_dtype(h, [&](auto t) {
        using T = decltype(t);
        // (fp32 stages are never deferred: an fp32 surrogate pair does not take the lazy branch, pend_f stays unused)
        return vjp_stage_t<T>(h, (const T*)p, (const T*)u, state, (const T*)lam, adj, (T*)lamJ, (T*)dp, batch,
                              (hipStream_t)stream, dp_assign, su_scale, sl_scale,
                              defer && std::is_same<T, double>::value);
    });
}

kanode_status kanode_internal_vjp_flush(kanode_handle* h, void* stream) { return vjp_flush(h, (hipStream_t)stream); }
void kanode_internal_vjp_discard(kanode_handle* h) {
    h->njobs = 0;
    h->pend_valid = false;
}
bool kanode_internal_pair_lazy(const kanode_handle* h) {
    return h->spec.rhs_kind == KANODE_RHS_CHAIN && surrogate_pair(h) && h->opt.pair_vjp && h->opt.pair_fuse;
}

// every workspace a stage / adjoint-stage call of this batch may need, allocated now
// (so the calls can be captured into a hipGraph)
kanode_status kanode_internal_prepare(kanode_handle* h, int64_t batch, hipStream_t st) {
    kanode_status s = check_handle(h);
    if (s != KANODE_OK) return s;
    if ((s = ensure_ws(h, batch, st)) != KANODE_OK) return s;
    if (h->spec.rhs_kind == KANODE_RHS_POINTWISE_PERIODIC_LAPLACIAN && (s = ensure_fk_ws(h, batch, st)) != KANODE_OK) return s;
    return ensure_stage_ws(h, 2 * (size_t)(h->n_in * batch) * h->esize, st);
}
