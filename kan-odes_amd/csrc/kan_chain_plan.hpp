// kan_chain_plan.hpp — what the host decides before it launches a small-chain kernel (host only, no HIP): whether a
// chain has the small-chain shape, which specialisation of the kernel serves it, and for the one-workgroup adjoint
// which model runs it, on how many threads, in how much dynamic LDS and with the dense output staged or not.
//
// Every launcher of kan_col.hip, kan_train.hip, kan_train_wg.hip, kan_ens_solve.hip, kan_traj_solve.hip, kan_traj_grad.hip and kan_traj_grad_f32.hip asks here, so the ensemble
// entries accept exactly the shapes the single launchers accept and the training loops carve LDS exactly as the
// adjoint launcher does.  LC is the layer-constants type (kan::LayerConst; a test passes its own struct with the
// same field names).  The numbers that belong to the device classes come in through ChainLimits, which kan_col.hip
// fills from its own constants (kChainLimits).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace kan {

struct ChainLimits {
    int dim, block, wave;              // kChainDim, kChainBlock, kWave
    int fwd_layers, vjp_layers;        // layers of the forward kernels (8) and of the pullback kernels (kChainMaxLayers)
    int max_batch, max_steps;          // kChainSolveMaxBatch, kChainAdjointMaxSteps
    int wide_f1, wide_f2, wide_end;    // kWideF1, kWideF2 (wide_fits), WideModel::kEnd
    int lv_I, lv_H, lv_O, lv_G, lv_P;  // LvWaveShape, kLvP
    int lv_sp, lv_sp_waves;            // KAN_LV_SP, kLvSpWaves
    size_t lc_bytes;                   // sizeof(LayerConst)
    int norm_tanh_fast, norm_softsign, path_rec, path_rec_corr, basis_rbf;   // the enumerators of kan_device.hpp
};

constexpr size_t kChainParamBudget = 48 * 1024;   // the constants and parameters of a forward kernel
constexpr size_t kOneWgBudget = 60 * 1024;        // a one-workgroup adjoint of up to four waves
constexpr size_t kLvSpBudget = 140 * 1024;        // the stage-parallel adjoint and the training loops

// ---- the small-chain shape ------------------------------------------------------------------------------------
// 1 <= nl <= max_layers, every layer at most `dim` wide, one normalizer / path specialisation, consecutive layers fit
template <class LC>
bool chain_small_layers(const ChainLimits& k, const LC* hlcs, int nl, int max_layers) {
    if (nl < 1 || nl > max_layers) return false;
    for (int l = 0; l < nl; ++l) {
        const LC& h = hlcs[l];
        if (h.I > k.dim || h.O > k.dim || h.path != hlcs[0].path || h.norm != hlcs[0].norm) return false;
        if (l > 0 && h.I != hlcs[l - 1].O) return false;
    }
    return true;
}
template <class LC>
bool I_ne_O(const LC* hlcs, int nl) { return hlcs[0].I != hlcs[nl - 1].O; }
inline bool chain_batch_ok(const ChainLimits& k, int64_t B) { return B >= 1 && B <= k.max_batch; }
inline bool chain_steps_ok(const ChainLimits& k, int64_t steps) { return steps >= 1 && steps <= k.max_steps; }
// the constants and the parameters, as every forward kernel stages them in LDS
inline size_t chain_param_lds(const ChainLimits& k, int nl, int64_t P, size_t esize) {
    return nl * k.lc_bytes + (size_t)P * esize;
}
inline bool chain_params_fit(const ChainLimits& k, int nl, int64_t P, size_t esize) {
    return chain_param_lds(k, nl, P, esize) <= kChainParamBudget;
}
// the block of a one-workgroup kernel on ChainModel: `dim` lanes per trajectory, whole waves
inline int chain_threads(const ChainLimits& k, int64_t B) { return (int)((B * k.dim + k.wave - 1) / k.wave) * k.wave; }
// what the one-workgroup solve covers (kd_chain_tsit5_kernel and its ensemble twin)
template <class LC>
bool chain_tsit5_shape(const ChainLimits& k, const LC* hlcs, int nl, int64_t P, int64_t B, size_t esize) {
    return chain_small_layers(k, hlcs, nl, k.fwd_layers) && chain_batch_ok(k, B) && !I_ne_O(hlcs, nl) &&
           chain_params_fit(k, nl, P, esize);
}

template <class LC>
bool chain_is_lv(const LC* hlcs, int nl) {
    return nl == 2 && hlcs[0].I == 2 && hlcs[0].O == 10 && hlcs[1].I == 10 && hlcs[1].O == 2 && hlcs[0].G == 5 &&
           hlcs[1].G == 5;
}

// ---- the specialisation ladder --------------------------------------------------------------------------------
// The rung of a small chain's kernel (its NORM, PATH and shape-class template arguments; chain_ladder in kan_col.hip
// turns the rung into compile-time tags).  hlcs passes chain_small_layers: layer 0 speaks for all.
enum ChainRung : int {
    kRungLV = 0,        // NORM_TANH_FAST, PATH_REC, ChainShapeLV
    kRungTanhRec = 1,   // NORM_TANH_FAST, PATH_REC, ChainShapeAny
    kRungRecCorr = 2,   // NORM_RUNTIME, PATH_REC_CORR, ChainShapeAny
    kRungRec = 3,       // NORM_RUNTIME, PATH_REC, ChainShapeAny
    kRungDirect = 4     // NORM_RUNTIME, PATH_DIRECT, ChainShapeAny
};
template <class LC>
ChainRung chain_rung(const ChainLimits& k, const LC* hlcs, int nl) {
    const LC& h = hlcs[0];
    if (h.norm == k.norm_tanh_fast && h.path == k.path_rec) return chain_is_lv(hlcs, nl) ? kRungLV : kRungTanhRec;
    if (h.path == k.path_rec_corr) return kRungRecCorr;
    return h.path == k.path_rec ? kRungRec : kRungDirect;
}

// ---- the one-workgroup adjoint --------------------------------------------------------------------------------
// one trajectory of a two-layer chain with base activations under one of the two normalizers the wave / workgroup
// models are compiled for
template <class LC>
bool chain_is_one_wide(const ChainLimits& k, const LC* hlcs, int nl, int64_t B, bool wide) {
    return wide && B == 1 && nl == 2 && hlcs[0].use_base && hlcs[1].use_base && hlcs[0].norm == hlcs[1].norm &&
           (hlcs[0].norm == k.norm_tanh_fast || hlcs[0].norm == k.norm_softsign);
}
// ... of the Lotka-Volterra shape: the chain on one wave (LvWaveModel: the lvsp / lvwave adjoints, the fused
// training loop)
template <class LC>
bool chain_is_lv_wave(const ChainLimits& k, const LC* hlcs, int nl, int64_t B, bool wide) {
    return chain_is_one_wide(k, hlcs, nl, B, wide) && hlcs[0].I == k.lv_I && hlcs[0].O == k.lv_H &&
           hlcs[1].I == k.lv_H && hlcs[1].O == k.lv_O && hlcs[0].G == k.lv_G && hlcs[1].G == k.lv_G &&
           hlcs[0].basis == k.basis_rbf && hlcs[1].basis == k.basis_rbf;
}
// ... [I -> H -> O] whose features fit the workgroup of WideModel: a DPP row per hidden unit, a wave per output
inline bool wide_fits(const ChainLimits& k, int I, int H, int O, int G1, int G2) {
    return I >= 1 && O >= 1 && I == O && H <= k.block / k.wide_f1 && I * (G1 + 1) <= k.wide_f1 &&
           H * (G2 + 1) <= k.wide_f2 && O <= k.block / k.wave;
}
template <class LC>
bool chain_is_wide(const ChainLimits& k, const LC* hlcs, int nl, int64_t B, bool wide) {
    return chain_is_one_wide(k, hlcs, nl, B, wide) && hlcs[1].I == hlcs[0].O &&
           wide_fits(k, hlcs[0].I, hlcs[0].O, hlcs[1].O, hlcs[0].G, hlcs[1].G);
}

// the forward's dense output of `steps` steps (seven stages each, and k1 of the first) of n entries
inline size_t onewg_rec_bytes(int64_t steps, int64_t n, size_t esize) {
    return esize * ((size_t)steps * 7 + 1) * (size_t)n;
}
// LvWaveModel and WideModel: `pre` bytes (the constants, ps, μ [2], kμ [7], the model's scratch), then t and dt of
// every step, then the dense output where all of it stays within the budget.  0: does not fit.
inline size_t onewg_staged_lds(size_t pre, int64_t steps, size_t rec, int* stage_rec) {
    size_t lds = pre + 2 * sizeof(double) * (size_t)steps;
    *stage_rec = lds + rec <= kOneWgBudget ? 1 : 0;
    if (*stage_rec) lds += rec;
    return pre % 8 == 0 && lds <= kOneWgBudget ? lds : 0;
}
// The stage-parallel Lotka-Volterra adjoint (fp64): the constants, ps, t and dt of every step and `extra` doubles
// of the caller's (the training loop's saveat rows), then the dense output where it fits beside the kernel's static
// Jacobian stage (jst).  0: does not fit.
inline size_t lvsp_lds(const ChainLimits& k, int64_t steps, size_t extra, int* stage_rec) {
    const size_t jst = sizeof(double) * 8 * k.lv_I * (k.lv_P + k.lv_I);
    const size_t rec = onewg_rec_bytes(steps, k.lv_I, sizeof(double));
    size_t lsp = 2 * k.lc_bytes + sizeof(double) * (k.lv_P + 2 * (size_t)steps + extra);
    *stage_rec = lsp + rec + jst <= kLvSpBudget ? 1 : 0;
    if (*stage_rec) lsp += rec;
    return lsp + jst <= kLvSpBudget ? lsp : 0;
}
// ChainModel: the constants, ps, a gradient row per column group, μ [2], kμ [7], t and dt of every step
inline size_t chain_group_adjoint_lds(const ChainLimits& k, int nl, int64_t P, int64_t B, int64_t steps, size_t esize) {
    const int NG = chain_threads(k, B) / k.dim;
    const size_t lds = nl * k.lc_bytes + (size_t)P * esize * (1 + NG + 9) + 2 * sizeof(double) * (size_t)steps + 16;
    return lds <= kOneWgBudget && ((size_t)P * esize) % 8 == 0 ? lds : 0;
}

enum ChainAdjModel : int { kAdjNone = 0, kAdjLvSp, kAdjLvWave, kAdjWide, kAdjChain };
struct ChainAdjPlan {
    int model, threads;
    size_t lds;      // dynamic LDS of the launch
    int stage_rec;   // the dense output is staged in it
};
// The model that runs the InterpolatingAdjoint of `steps` forward steps in one workgroup, the first that fits:
// the stage-parallel Lotka-Volterra kernel, the LV wave, the whole workgroup on one trajectory, a column group per
// trajectory.  A training loop passes its capacity as steps (what holds at cap holds at every count the loop can
// reach) and lv_models = false where its kernel has no LvWaveModel.
template <class LC>
ChainAdjPlan chain_adjoint_plan(const ChainLimits& k, const LC* hlcs, int nl, int64_t P, int64_t B, bool wide,
                                int64_t steps, size_t esize, bool lv_models = true) {
    const ChainAdjPlan none{kAdjNone, 0, 0, 0};
    if (nl < 1 || nl > k.vjp_layers || !chain_batch_ok(k, B) || I_ne_O(hlcs, nl) || !chain_steps_ok(k, steps))
        return none;
    int sr = 0;
    if (lv_models && chain_is_lv_wave(k, hlcs, nl, B, wide)) {
        if (esize == sizeof(double) && k.lv_sp && P == k.lv_P)
            if (const size_t lds = lvsp_lds(k, steps, 0, &sr)) return {kAdjLvSp, (k.lv_sp_waves + 1) * k.wave, lds, sr};
        const size_t pre = 2 * k.lc_bytes + esize * (size_t)P * 10;
        if (const size_t lds = onewg_staged_lds(pre, steps, onewg_rec_bytes(steps, k.lv_I, esize), &sr))
            return {kAdjLvWave, k.wave, lds, sr};
    }
    if (chain_is_wide(k, hlcs, nl, B, wide)) {
        const size_t pre = 2 * k.lc_bytes + esize * ((size_t)P * 10 + k.wide_end);
        if (const size_t lds = onewg_staged_lds(pre, steps, onewg_rec_bytes(steps, hlcs[0].I, esize), &sr))
            return {kAdjWide, k.block, lds, sr};
    }
    if (!chain_small_layers(k, hlcs, nl, k.vjp_layers)) return none;
    if (const size_t lds = chain_group_adjoint_lds(k, nl, P, B, steps, esize))
        return {kAdjChain, chain_threads(k, B), lds, 0};
    return none;
}

// ---- the fp32 trajectory gradient (kan_traj_grad_f32.hip) -----------------------------------------------------
// The dynamic LDS of one trajectory's workgroup (one wave, `groups` = wave / dim column groups), in BYTES after the
// layer constants: ps [P] | rows [groups][P] | μ [2][P] | kμ [7][P] | the gradient [P] (floats; rows, μ and kμ
// contiguous, zeroed together as kd_chain_adjoint_kernel zeroes them) | ts, dts [cap] each | saveat [n_save] (doubles)
// | (dl_lds) u_save / dl [n_save][n] (floats).  The doubles start at a multiple of 8 bytes where 4·P is one (P even)
// and the constants' bytes are.  (constexpr: the kernel carves with the same function.)
struct TrajGradF32Carve {
    size_t ps, work, mu, km, gl, tsl, dtsl, sv, dl, total;
};
constexpr TrajGradF32Carve traj_grad_f32_carve(int64_t P, int64_t groups, int64_t cap, int64_t n_save, int64_t n,
                                               int dl_lds) {
    TrajGradF32Carve c{};
    const size_t f = sizeof(float), d = sizeof(double);
    size_t o = 0;
    c.ps = o, o += f * (size_t)P;
    c.work = o, o += f * (size_t)(groups * P);
    c.mu = o, o += f * (size_t)(2 * P);
    c.km = o, o += f * (size_t)(7 * P);
    c.gl = o, o += f * (size_t)P;
    c.tsl = o, o += d * (size_t)cap;
    c.dtsl = o, o += d * (size_t)cap;
    c.sv = o, o += d * (size_t)n_save;
    c.dl = o, o += dl_lds ? f * (size_t)(n_save * n) : 0;
    c.total = o;
    return c;
}
// The whole dynamic LDS of a launch with a dense output of `cap` steps, within kOneWgBudget; *dl_lds: u_save / dl live
// in it (else in the trajectory's global block).  0: not covered (layers wider than `dim`, more layers than the
// pullback takes, n_in != n_out, odd P: chain_group_adjoint_lds asks for (4·P) % 8 == 0) or no fit.  The adjoint is
// the column-group model on one wave: chain_adjoint_plan at B = 1 with wide = false must give kAdjChain on `wave`
// threads.
template <class LC>
size_t traj_grad_f32_lds(const ChainLimits& k, const LC* hlcs, int nl, int64_t P, int64_t cap, int64_t n_save,
                         int* dl_lds) {
    if (dl_lds) *dl_lds = 0;
    if (nl < 1 || n_save < 0 || cap < 1 || !chain_small_layers(k, hlcs, nl, k.vjp_layers) ||
        !chain_params_fit(k, nl, P, sizeof(float)) || (nl * k.lc_bytes) % 8 || (P * sizeof(float)) % 8)
        return 0;
    const ChainAdjPlan plan = chain_adjoint_plan(k, hlcs, nl, P, 1, false, cap, sizeof(float), false);
    if (plan.model != kAdjChain || plan.threads != k.wave) return 0;
    const int64_t n = hlcs[0].I;
    auto bytes = [&](int dl) {
        return nl * k.lc_bytes + traj_grad_f32_carve(P, k.wave / k.dim, cap, n_save, n, dl).total;
    };
    if (bytes(0) > kOneWgBudget) return 0;
    const int dl = bytes(1) <= kOneWgBudget ? 1 : 0;
    if (dl_lds) *dl_lds = dl;
    return bytes(dl);
}

}  // namespace kan
