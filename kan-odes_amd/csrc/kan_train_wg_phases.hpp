// kan_train_wg_phases.hpp — the phases of one training iteration of a small chain on one workgroup, shared by the
// kernels that run them: kd_chain_train_wg_kernel and its ensemble twin (kan_train_wg.hip: K iterations with Adam) and
// kd_chain_traj_grad_kernel (kan_traj_grad.hip: one solve, loss and adjoint per trajectory, no loop).  Device only:
// include after kan_col.hip (KAN_COL_DEVICE_ONLY) and kan_train_loss.hpp.  The LDS carve and the pointers every phase
// reads are here as well, so each kernel lays its LDS out the same way.
#pragma once

namespace kan {

enum TrainWgModel : int { kWgNone = 0, kWgChain = 1, kWgWide = 2 };

// LDS of a launch, in doubles after the layer constants: ps [P] | work (ChainModel: rows [NG][P]; WideModel: its
// scratch) | μ [2][P] | kμ [7][P] | the gradient [P] | ts, dts [cap] each | saveat [n_save] | the test saveat
// [n_save_test] | (dl_lds) u_save / dl [n_save][n], the test u_save [n_save_test][n] | (stage_rec) the dense output
// [(7 cap + 1) n].  work, μ and kμ are contiguous (zeroed together, as the adjoint kernels do).
struct TrainWgCarve {
    size_t ps, work, mu, km, gl, tsl, dtsl, sv, svt, dl, ust, recl, total;   // doubles, from the end of the constants
};
__host__ __device__ inline TrainWgCarve train_wg_carve(int64_t P, int64_t work, int64_t cap, int64_t n_save,
                                                       int64_t n_save_test, int64_t n, int dl_lds, int stage_rec) {
    TrainWgCarve c{};
    size_t o = 0;
    c.ps = o, o += P;
    c.work = o, o += work;
    c.mu = o, o += 2 * P;
    c.km = o, o += 7 * P;
    c.gl = o, o += P;
    c.tsl = o, o += cap;
    c.dtsl = o, o += cap;
    c.sv = o, o += n_save;
    c.svt = o, o += n_save_test;
    c.dl = o, o += dl_lds ? n_save * n : 0;
    c.ust = o, o += dl_lds ? n_save_test * n : 0;
    c.recl = o, o += stage_rec ? (cap * 7 + 1) * n : 0;
    c.total = o;
    return c;
}

// what every phase needs besides the launch's arguments: pointers into LDS, typed as such (a phase is a function of
// its own, and through a plain pointer argument it would read LDS with flat loads), and the global dense-output block
#define KAN_LDS __attribute__((address_space(3)))
struct TrainWgPtrs {
    KAN_LDS const double* tab;       // the exp table
    KAN_LDS const LayerConst* lcl;
    KAN_LDS double *ps, *work, *mu, *km, *gl, *tsl, *dtsl, *sv, *svt, *recl;
    double *dl, *ust;        // u_save / dl and the test u_save: LDS (dl_lds) or global
    double *rec, *rk1;       // global: [cap][7][n], k1_0 [n]
    KAN_LDS double* red;     // onewg_bsum's partials
    KAN_LDS int64_t* fo;     // [3][4]: the counters of the training forward, the test solve, the adjoint
    KAN_LDS double* lossv;   // loss[it]
    int nl, P;
};

// A value every lane holds alike, moved to scalar registers.  The phases read their arguments from private memory
// (structs passed by reference to functions that are not inlined), where the compiler cannot know that they are
// wave-uniform: without this every solver option is a vector register and every step-control branch a vector branch.
template <typename T>
__device__ __forceinline__ T wg_uniform(T v) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "one or two scalar registers");
    int x[sizeof(T) / 4];
    __builtin_memcpy(x, &v, sizeof(T));
#pragma unroll
    for (int i = 0; i < (int)(sizeof(T) / 4); ++i) x[i] = __builtin_amdgcn_readfirstlane(x[i]);
    __builtin_memcpy(&v, x, sizeof(T));
    return v;
}

// A: the solve at p_it over (t0, tf), dense output kept, or (tst) the test solve over (t0, tf_test)
template <int FN, int PATH, class FS>
__device__ __noinline__ void wg_forward(const ChainTrainArgs& a, const TrainWgPtrs& L, bool tst_) {
    const bool tst = wg_uniform((int)tst_) != 0;
    ChainSolveArgs fa{};
    fa.t0 = wg_uniform(a.t0);
    fa.tf = wg_uniform(tst ? a.tf_test : a.tf);
    fa.dt = wg_uniform(a.dt);
    fa.abstol = wg_uniform(a.abstol);
    fa.reltol = wg_uniform(a.reltol);
    fa.dtmin = wg_uniform(a.dtmin);
    fa.beta1 = wg_uniform(a.beta1);
    fa.beta2 = wg_uniform(a.beta2);
    fa.gamma = wg_uniform(a.gamma);
    fa.qmin = wg_uniform(a.qmin);
    fa.qmax = wg_uniform(a.qmax);
    fa.qoldinit = wg_uniform(a.qoldinit);
    fa.adaptive = wg_uniform(a.adaptive);
    fa.maxiters = wg_uniform(a.maxiters);
    fa.n_save = wg_uniform(tst ? a.n_save_test : a.n_save);
    fa.cap = wg_uniform(a.cap);
    fa.saveat = (const double*)wg_uniform(tst ? L.svt : L.sv);
    fa.u_save = wg_uniform(tst ? L.ust : L.dl);
    fa.rec = wg_uniform(tst ? (double*)nullptr : L.rec);
    fa.k1_0 = wg_uniform(L.rk1);
    fa.ts = (double*)wg_uniform(L.tsl);
    fa.dts = (double*)wg_uniform(L.dtsl);
    fa.out = (int64_t*)wg_uniform(L.fo) + (tst ? 4 : 0);
    const Math<double> M{(const double*)wg_uniform(L.tab)};
    const int N = wg_uniform((int)a.N), nl = wg_uniform(L.nl), P = wg_uniform(L.P);
    const int64_t B = wg_uniform(a.B);
    const int j = threadIdx.x & (kChainDim - 1);
    const int64_t col = threadIdx.x / kChainDim;
    ChainModel<double, FN, PATH, FS> m{M, (const LayerConst*)wg_uniform(L.lcl), nl, (const double*)wg_uniform(L.ps),
                                       nullptr, P, j, 0, col < B && j < N, (int64_t)N * col + j, (int64_t)N * B};
    onewg_tsit5<double>(m, wg_uniform(a.u0), fa, (double*)wg_uniform(L.red));
}

// A: loss[it] and the cotangent in place of u_save, on wave 0
__device__ __noinline__ void wg_loss(const ChainTrainArgs& a, const TrainWgPtrs& L, int64_t it) {
    if (threadIdx.x >= kWave) return;
    double lv = wave_mse<true>(L.dl, a.target, a.n_save * a.N * a.B, a.dl_scale);
    if (a.act_reg != 0.0) lv = l1_loss(lv, (const double*)L.ps, L.P, a.act_reg);   // (λ = 0: not one operation more)
    if (threadIdx.x == 0) {
        a.loss[it] = lv;
        *L.lossv = lv;
    }
}

// A: loss_test[it - 1] from the test solve just run, on wave 0
__device__ __noinline__ void wg_test_loss(const ChainTrainArgs& a, const TrainWgPtrs& L, int64_t it) {
    if (threadIdx.x >= kWave) return;
    const double lt = wave_mse<false>(L.ust, a.target_test, a.n_save_test * a.N * a.B, 0.0);
    if (threadIdx.x == 0) a.loss_test[it - 1] = L.fo[7] == 0 ? lt : __longlong_as_double(0x7ff8000000000000LL);
}

// (the generic shapes are too large for the stage loops to be unrolled, as in kan_col.hip's adjoint kernels)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wpass-failed"
// B: the InterpolatingAdjoint from the dense output just written; the gradient -> L.gl, the counters -> L.fo[8..]
// ADJ: kWgChain (ChainModel<FN, PATH, FS>, as kd_chain_adjoint_kernel) or kWgWide (WideModel<WN>, as
// kd_chain_adjoint_wide_kernel).  The text is kan_train_wg_adjoint.inc.
template <int ADJ, int WN, int FN, int PATH, class FS>
__device__ __noinline__ void wg_adjoint(const ChainTrainArgs& a, const TrainWgPtrs& L) {
#define KAN_WG_ADJOINT_DU0
#include "kan_train_wg_adjoint.inc"
#undef KAN_WG_ADJOINT_DU0
}
#pragma clang diagnostic pop

}  // namespace kan
