// kan_train.hip — K whole training iterations of one Lotka-Volterra trajectory in ONE launch (gfx950).
//
// The reference's driver loop (LV_driver_KANODE.jl:279-291) is, per iteration, a forward solve, the loss, the
// InterpolatingAdjoint, Flux's Adam update and the test-loss solve.  The forward solve and the adjoint were one
// workgroup each already (kd_chain_tsit5_kernel, kd_chain_adjoint_lvsp_kernel); nothing between them depends on
// the host (u0, tspan, saveat, the target, the jump groups and the options are the same every iteration, only p
// and the Adam moments change), so here the whole loop stays on the device and the host launches once per chunk
// of iterations.
//
// One workgroup of (kLvSpWaves + 1) waves, as the lvsp adjoint.  Per iteration `it`:
//   A  wave 0: the forward solve at p_it over (t0, tf) (onewg_tsit5 in its wave-local mode with ChainModel: the
//      arithmetic of kd_chain_tsit5_kernel), the dense output into LDS (or global when cap steps do not fit),
//      then loss[it] (with a penalty weight λ = act_reg: + λ·Σ|p|, the driver's sparse_on = 1 loss) and
//      dl = (u_save - X)·2/numel in place of u_save;
//      wave 1, at the same time and at the same p_it: the test-loss solve over (t0, tf_test) -> loss_test[it-1]
//      (the test solve of iteration it-1 is the solve at p_it = p_{(it-1)+1}; the last one runs alone after the
//      loop).  Waves 2..6 wait at the barrier.
//   -- barrier; every thread reads the solves' status words and stops the loop on a failure
//   B  all waves: lvsp_adjoint (its own barriers: 2 per attempted step, + 2 for the initial step)
//   C  wave 0: the gradient μ (+ λ·sgn(p) with a penalty), the optional records (counts, grad, p_before), then
//      Adam on its entries (adam_entry: the
//      statement of adam_step_kernel) -> p (global and the LDS copy), m, v
//   -- barrier; βp1, βp2 advance by one product in every thread
// so two barriers per iteration besides the adjoint's.
#define KAN_COL_DEVICE_ONLY
#include "kan_col.hip"
#include "kan_train_loss.hpp"   // wave_mse, l1_loss (shared with kan_train_wg.hip)

namespace kan {

// NORM: the adjoint's normalizer; FN, PATH, FS: the forward's ChainModel specialisation (what
// launch_kd_chain_tsit5 picks for the handle)
template <int NORM, int FN, int PATH, class FS>
__global__ void __launch_bounds__((kLvSpWaves + 1) * kWave)
kd_chain_train_lvsp_kernel(const LayerConst* __restrict__ lcs, ChainTrainArgs a) {
#include "kan_train_body.inc"
}

// The ensemble entry: workgroup r runs the loop on args[r] (its own p, m, v, Adam scalars, records, dense-output
// block and status words; the problem, the jump groups and the options are the same in every struct).  The
// workgroups share nothing they write and never wait for each other; one that stops writes its own status words
// and returns.
template <int NORM, int FN, int PATH, class FS>
__global__ void __launch_bounds__((kLvSpWaves + 1) * kWave)
kd_chain_train_lvsp_ens_kernel(const LayerConst* __restrict__ lcs, const ChainTrainArgs* __restrict__ args) {
    const ChainTrainArgs a = args[blockIdx.x];
#include "kan_train_body.inc"
}

bool chain_train_supported(const LayerConst* hlcs, int nl, int64_t P, int64_t B, size_t esize, bool wide) {
    // (one path specialisation for both layers: launch_kd_chain_tsit5's condition, whose arithmetic the forward is)
    return KAN_LV_SP && esize == sizeof(double) && P == kLvP && chain_is_lv_wave(kChainLimits, hlcs, nl, B, wide) &&
           hlcs[0].path == hlcs[1].path;
}

// the stage-parallel adjoint's LDS at cap steps, with the saveat times and rows of both problems beside it
size_t chain_train_lds(int64_t cap, int64_t n_save, int64_t n_save_test, int* stage_rec) {
    int sr = 0;
    const size_t lds = lvsp_lds(kChainLimits, cap, (size_t)(1 + LvWaveShape::I) * (n_save + n_save_test), &sr);
    if (stage_rec) *stage_rec = sr;
    return lds;
}

// args == nullptr: the single-replica kernel on `a`; else the ensemble kernel, one workgroup per struct of the device
// array args [n_rep] (a: the host copy of any one of them -- they agree in every field read here)
static hipError_t launch_chain_train(const LayerConst* hlcs, int nl, const LayerConst* lcs, int64_t P,
                                     const ChainTrainArgs& a, const ChainTrainArgs* args, int64_t n_rep,
                                     hipStream_t st) {
    if (!chain_train_supported(hlcs, nl, P, 1, sizeof(double), true) || a.cap < 1 || a.cap > kChainAdjointMaxSteps ||
        a.n_iters < 1 || a.n_save < 0 || a.n_save_test < 0 || (args && (n_rep < 1 || n_rep > kTrainMaxReplicas)))
        return hipErrorNotSupported;
    int sr = 0;
    const size_t lds = chain_train_lds(a.cap, a.n_save, a.n_save_test, &sr);
    if (lds == 0 || sr != a.stage_rec || (!sr && !a.rec)) return hipErrorNotSupported;
    const LayerConst& h = hlcs[0];
    const bool tf = h.norm == NORM_TANH_FAST;
    // the forward's specialisation is the handle's rung of chain_ladder, paired here with the adjoint's normalizer:
    // only these six combinations exist, so the ladder stays written out
#define KAN_TRAIN_GO(NORM, FN, PATH, FS)                                                                            \
    do {                                                                                                            \
        const void* fn = args ? reinterpret_cast<const void*>(&kd_chain_train_lvsp_ens_kernel<NORM, FN, PATH, FS>)  \
                              : reinterpret_cast<const void*>(&kd_chain_train_lvsp_kernel<NORM, FN, PATH, FS>);     \
        const hipError_t e = ensure_dynamic_lds(fn, lds);                                                           \
        if (e != hipSuccess) return e;                                                                              \
        if (args)                                                                                                   \
            hipLaunchKernelGGL((kd_chain_train_lvsp_ens_kernel<NORM, FN, PATH, FS>), dim3((unsigned)n_rep),         \
                               dim3((kLvSpWaves + 1) * kWave), lds, st, lcs, args);                                 \
        else                                                                                                        \
            hipLaunchKernelGGL((kd_chain_train_lvsp_kernel<NORM, FN, PATH, FS>), dim3(1),                           \
                               dim3((kLvSpWaves + 1) * kWave), lds, st, lcs, a);                                    \
    } while (0)
    if (tf && h.path == PATH_REC) KAN_TRAIN_GO(NORM_TANH_FAST, NORM_TANH_FAST, PATH_REC, ChainShapeLV);
    else if (tf && h.path == PATH_REC_CORR) KAN_TRAIN_GO(NORM_TANH_FAST, NORM_RUNTIME, PATH_REC_CORR, ChainShapeAny);
    else if (tf) KAN_TRAIN_GO(NORM_TANH_FAST, NORM_RUNTIME, PATH_DIRECT, ChainShapeAny);
    else if (h.path == PATH_REC) KAN_TRAIN_GO(NORM_SOFTSIGN, NORM_RUNTIME, PATH_REC, ChainShapeAny);
    else if (h.path == PATH_REC_CORR) KAN_TRAIN_GO(NORM_SOFTSIGN, NORM_RUNTIME, PATH_REC_CORR, ChainShapeAny);
    else KAN_TRAIN_GO(NORM_SOFTSIGN, NORM_RUNTIME, PATH_DIRECT, ChainShapeAny);
#undef KAN_TRAIN_GO
    return hipGetLastError();
}

hipError_t launch_kd_chain_train(const LayerConst* hlcs, int nl, const LayerConst* lcs, int64_t P,
                                 const ChainTrainArgs& a, hipStream_t st) {
    return launch_chain_train(hlcs, nl, lcs, P, a, nullptr, 1, st);
}

hipError_t launch_kd_chain_train_ensemble(const LayerConst* hlcs, int nl, const LayerConst* lcs, int64_t P,
                                          const ChainTrainArgs& a, const ChainTrainArgs* args, int64_t n_rep,
                                          hipStream_t st) {
    return args ? launch_chain_train(hlcs, nl, lcs, P, a, args, n_rep, st) : hipErrorNotSupported;
}

}  // namespace kan
