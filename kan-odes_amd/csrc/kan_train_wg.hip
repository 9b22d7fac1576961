// kan_train_wg.hip — K whole training iterations of a small chain in ONE launch (gfx950), for every shape the
// one-workgroup forward and adjoint cover that kan_train.hip's Lotka-Volterra kernel does not: a pruned [2,k,2],
// a [3,6,3] chain, three layers, up to kChainSolveMaxBatch trajectories (KANODE_OPT_TRAIN_ANY_CHAIN), and its ensemble
// twin, R such loops in one launch, one workgroup each (kanode_fit_ensemble_tsit5).  The loop's text is
// kan_train_wg_body.inc, included into both kernels; the phase functions are kan_train_wg_phases.hpp, shared with
// kan_traj_grad.hip.
//
// The loop is LV_driver_KANODE.jl:279-291, as in kan_train.hip; here every phase runs on the whole workgroup, with
// the device functions of the two-launch path (kan_onewg.hpp on the model classes of kan_col.hip).  Per iteration it:
//   A  wg_forward: onewg_tsit5 in block mode on ChainModel (kd_chain_tsit5_kernel's arithmetic) at p_it; the dense
//      output [step][u_n, k_2..k_7][N·B] and k1_0 go to global memory (ChainTrainArgs::rec), ts / dts stay in LDS.
//      barrier.  wg_loss (wave 0): loss[it] = wave_mse (+ l1_loss with a penalty), u_save <- dl = (u - X)·2/numel.
//      With a test problem and it > 0: wg_forward again over (t0, tf_test) at the same p_it, barrier, wg_test_loss
//      -> loss_test[it - 1] (the last one after the loop).
//   -- barrier; every thread reads the status words and takes the same stop decision
//   B  wg_adjoint: onewg_adjoint on the model launch_kd_chain_adjoint picks: WideModel (one trajectory of a
//      two-layer chain that passes wide_fits; block of kChainBlock) or ChainModel (block of ⌈16 B / 64⌉ waves), with
//      that launcher's LDS carve (rows or the Wide scratch, μ [2][P], kμ [7][P]); WideModel copies the dense output
//      into LDS first where it fits in that launcher's 60 KB.  The gradient μ goes to LDS.
//   -- barrier
//   C  wg_adam: the records (counts, grad, p_before), the gradient μ (+ λ·sgn(p)), adam_entry per parameter
//      spread over the block -> p (global and the LDS copy), m, v
//   -- barrier; βp1, βp2 advance by one rounded product in every thread
// The forward runs in the adjoint's block: at B = 1 under WideModel that is four waves where kd_chain_tsit5_kernel
// has one; onewg_bsum then adds the idle waves' zeros, which changes no bit of a sum of squares.
// The global dense output is written in A and read in B by the same workgroup; the barrier between them (a
// workgroup-scope release / acquire, with the stores waited for) orders them, as for kan_train_body.inc's global
// record.  Each phase is a function of its own (not inlined): a phase's registers are then not live across the
// others (DESIGN §7 on the 368 B/lane of scratch of the one-body LV kernel).
#define KAN_COL_DEVICE_ONLY
#include "kan_col.hip"
#include "kan_train_loss.hpp"
#include "kan_train_wg_phases.hpp"

namespace kan {

// C: the records and Adam, parameter q on thread q mod blockDim
__device__ __noinline__ void wg_adam(const ChainTrainArgs& a, const TrainWgPtrs& L, int64_t it, double bp1, double bp2) {
    const int P = L.P;
    if (a.counts && threadIdx.x == 0) {
        a.counts[4 * it] = L.fo[0];
        a.counts[4 * it + 1] = L.fo[1];
        a.counts[4 * it + 2] = L.fo[8];
        a.counts[4 * it + 3] = L.fo[9];
    }
    AdamArgs ad;
    ad.scale = 1.0;
    ad.beta1 = a.ab1;
    ad.beta2 = a.ab2;
    ad.omb1 = a.omb1;
    ad.omb2 = a.omb2;
    {   // (contraction off: 1 - βp must not fuse with the product that advanced βp)
#pragma clang fp contract(off)
        ad.c1 = 1.0 - bp1;
        ad.c2 = 1.0 - bp2;
    }
    ad.eps = a.eps;
    ad.eta = a.eta;
    for (int q = threadIdx.x; q < P; q += blockDim.x) {
        const double x = L.ps[q];
        double gq = L.gl[q];
        // ∂(λ·Σ|p|)/∂p_q = λ·sgn(p_q), sgn(0) = 0: one rounded add (λ = 0: none, a -0.0 stays -0.0)
        if (a.act_reg != 0.0) gq = __dadd_rn(gq, x > 0.0 ? a.act_reg : (x < 0.0 ? -a.act_reg : 0.0));
        if (a.grad) a.grad[it * P + q] = gq;
        if (a.p_before) a.p_before[it * P + q] = x;
        double mq = a.m[q], vq = a.v[q];
        const double xn = adam_entry<double>(x, mq, vq, gq, ad);
        a.m[q] = mq;
        a.v[q] = vq;
        a.p[q] = xn;
        L.ps[q] = xn;
    }
}

// FN, PATH, FS: the forward's ChainModel specialisation (the handle's rung of chain_ladder), which is the ChainModel
// adjoint's too; ADJ, WN: the adjoint's model
template <int FN, int PATH, class FS, int ADJ, int WN>
__global__ void __launch_bounds__(kChainBlock)
kd_chain_train_wg_kernel(const LayerConst* __restrict__ lcs, int nl, int P, ChainTrainArgs a) {
#include "kan_train_wg_body.inc"
}

// The ensemble twin (kanode_fit_ensemble_tsit5): workgroup r runs the same loop on its copy of args[r] (its own p, m,
// v, Adam scalars, λ, records, private global block and status words; the problem, the jump groups, cap, dl_lds and
// stage_rec are the same in every struct, so the LDS carve is every workgroup's alike).  The copy is made once, ahead
// of the body's first barrier, from a uniform read-only address: scalar loads.  The block index is used for nothing
// else: the workgroups share nothing they write and never wait for each other, and one that stops writes its own two
// status words and returns.
template <int FN, int PATH, class FS, int ADJ, int WN>
__global__ void __launch_bounds__(kChainBlock)
kd_chain_train_wg_ens_kernel(const LayerConst* __restrict__ lcs, int nl, int P,
                             const ChainTrainArgs* __restrict__ args) {
    const ChainTrainArgs a = args[blockIdx.x];
#include "kan_train_wg_body.inc"
}

// The adjoint's model, block and staging: where the forward fits the one-workgroup solve (at any step count: it keeps
// no dense output of its own), the plan of the one-workgroup adjoint at `cap` steps.  Its WideModel or ChainModel:
// this kernel has no LvWaveModel (chain_train_wg_supported leaves that shape to kd_chain_train_lvsp_kernel).
static ChainAdjPlan train_wg_plan(const LayerConst* hlcs, int nl, int64_t P, int64_t B, bool wide, int64_t cap) {
    if (!chain_small_layers(kChainLimits, hlcs, nl, kChainLimits.vjp_layers) ||
        !chain_params_fit(kChainLimits, nl, P, sizeof(double)) || (nl * sizeof(LayerConst)) % 8)
        return ChainAdjPlan{kAdjNone, 0, 0, 0};
    return chain_adjoint_plan(kChainLimits, hlcs, nl, P, B, wide, cap, sizeof(double), false);
}

size_t chain_train_wg_rec_elems(int64_t n, int64_t cap, int64_t n_save, int64_t n_save_test) {
    return (size_t)((cap * 7 + 1) * n + (n_save + n_save_test) * n);
}

size_t chain_train_wg_lds(const LayerConst* hlcs, int nl, int64_t P, int64_t B, bool wide, int64_t cap, int64_t n_save,
                          int64_t n_save_test, int* dl_lds, int* stage_rec) {
    constexpr size_t kBudget = 140 * 1024 - 4096;   // chain_train_lds's, less the kernel's static LDS (the exp table)
    const ChainAdjPlan plan = train_wg_plan(hlcs, nl, P, B, wide, cap);
    int sr = plan.stage_rec;
    if (dl_lds) *dl_lds = 0;
    if (stage_rec) *stage_rec = 0;
    if (plan.model == kAdjNone || n_save < 0 || n_save_test < 0) return 0;
    const int64_t n = (int64_t)hlcs[0].I * B;
    const int64_t work = plan.model == kAdjWide ? (int64_t)kChainLimits.wide_end : (int64_t)(plan.threads / kChainDim) * P;
    const size_t lc = nl * sizeof(LayerConst);
    auto bytes = [&](int dl, int st) {
        return lc + sizeof(double) * train_wg_carve(P, work, cap, n_save, n_save_test, n, dl, st).total;
    };
    if (bytes(0, 0) > kBudget) return 0;
    const int dl = bytes(1, 0) <= kBudget ? 1 : 0;
    if (sr && bytes(dl, 1) > kBudget) sr = 0;
    if (dl_lds) *dl_lds = dl;
    if (stage_rec) *stage_rec = sr;
    return bytes(dl, sr);
}

bool chain_train_wg_supported(const LayerConst* hlcs, int nl, int64_t P, int64_t B, size_t esize, bool wide) {
    if (esize != sizeof(double) || nl < 1 || chain_is_lv_wave(kChainLimits, hlcs, nl, B, wide)) return false;
    return chain_train_wg_lds(hlcs, nl, P, B, wide, 1, 1, 0, nullptr, nullptr) != 0;
}

// args == nullptr: the single-replica kernel on `a`; else the ensemble kernel, one workgroup per struct of the device
// array args [n_rep] (a: the host copy of any one of them -- they agree in every field read here; each has a private
// block of its own in rec)
static hipError_t launch_train_wg(const LayerConst* hlcs, int nl, const LayerConst* lcs, int64_t P, int64_t B,
                                  bool wide, const ChainTrainArgs& a, const ChainTrainArgs* args, int64_t n_rep,
                                  hipStream_t st) {
    if (!chain_train_wg_supported(hlcs, nl, P, B, sizeof(double), wide) || a.n_iters < 1 || a.B != B ||
        a.N != hlcs[0].I || !a.rec || (args && (n_rep < 1 || n_rep > kTrainMaxReplicas)))
        return hipErrorNotSupported;
    int dl = 0, sr = 0;
    const size_t lds = chain_train_wg_lds(hlcs, nl, P, B, wide, a.cap, a.n_save, a.n_save_test, &dl, &sr);
    if (lds == 0 || dl != a.dl_lds || sr != a.stage_rec) return hipErrorNotSupported;
    const ChainAdjPlan plan = train_wg_plan(hlcs, nl, P, B, wide, a.cap);
    const int threads = plan.threads;
    const LayerConst& h = hlcs[0];
#define KAN_TWG_GO(FN, PATH, FS, ADJ, WN)                                                                            \
    do {                                                                                                            \
        const void* fn = args ? reinterpret_cast<const void*>(&kd_chain_train_wg_ens_kernel<FN, PATH, FS, ADJ, WN>) \
                              : reinterpret_cast<const void*>(&kd_chain_train_wg_kernel<FN, PATH, FS, ADJ, WN>);    \
        const hipError_t e = ensure_dynamic_lds(fn, lds);                                                           \
        if (e != hipSuccess) return e;                                                                              \
        if (args)                                                                                                   \
            hipLaunchKernelGGL((kd_chain_train_wg_ens_kernel<FN, PATH, FS, ADJ, WN>), dim3((unsigned)n_rep),        \
                               dim3(threads), lds, st, lcs, nl, (int)P, args);                                      \
        else                                                                                                        \
            hipLaunchKernelGGL((kd_chain_train_wg_kernel<FN, PATH, FS, ADJ, WN>), dim3(1), dim3(threads), lds, st,  \
                               lcs, nl, (int)P, a);                                                                 \
    } while (0)
    // the forward's specialisation is the ladder's rung.  Under WideModel the rung is paired with the adjoint's
    // normalizer and only the six combinations a handle reaches exist (a [2,10,2] G = 5 chain on the exact
    // recurrence under WideModel is the LV-wave shape: not this kernel's), so that half stays written out
    const bool tf = h.norm == NORM_TANH_FAST;
    if (plan.model == kAdjWide) {
        if (tf && h.path == PATH_REC) KAN_TWG_GO(NORM_TANH_FAST, PATH_REC, ChainShapeAny, kWgWide, NORM_TANH_FAST);
        else if (tf && h.path == PATH_REC_CORR) KAN_TWG_GO(NORM_RUNTIME, PATH_REC_CORR, ChainShapeAny, kWgWide, NORM_TANH_FAST);
        else if (tf) KAN_TWG_GO(NORM_RUNTIME, PATH_DIRECT, ChainShapeAny, kWgWide, NORM_TANH_FAST);
        else if (h.path == PATH_REC_CORR) KAN_TWG_GO(NORM_RUNTIME, PATH_REC_CORR, ChainShapeAny, kWgWide, NORM_SOFTSIGN);
        else if (h.path == PATH_REC) KAN_TWG_GO(NORM_RUNTIME, PATH_REC, ChainShapeAny, kWgWide, NORM_SOFTSIGN);
        else KAN_TWG_GO(NORM_RUNTIME, PATH_DIRECT, ChainShapeAny, kWgWide, NORM_SOFTSIGN);
    } else {
        const hipError_t e = chain_ladder(hlcs, nl, [&](auto norm, auto path, auto shape) {
            KAN_TWG_GO(norm(), path(), decltype(shape), kWgChain, NORM_RUNTIME);
            return hipSuccess;
        });
        if (e != hipSuccess) return e;
    }
#undef KAN_TWG_GO
    return hipGetLastError();
}

hipError_t launch_kd_chain_train_wg(const LayerConst* hlcs, int nl, const LayerConst* lcs, int64_t P, int64_t B,
                                    bool wide, const ChainTrainArgs& a, hipStream_t st) {
    return launch_train_wg(hlcs, nl, lcs, P, B, wide, a, nullptr, 1, st);
}

hipError_t launch_kd_chain_train_wg_ensemble(const LayerConst* hlcs, int nl, const LayerConst* lcs, int64_t P,
                                             int64_t B, bool wide, const ChainTrainArgs& a, const ChainTrainArgs* args,
                                             int64_t n_rep, hipStream_t st) {
    return args ? launch_train_wg(hlcs, nl, lcs, P, B, wide, a, args, n_rep, st) : hipErrorNotSupported;
}

#undef KAN_LDS

}  // namespace kan
