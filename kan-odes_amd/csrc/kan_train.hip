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

namespace kan {

// Σ_i (us[i] - X[i])² / cnt over the calling wave, us in LDS: lane l sums its terms l, l + 64, .. in order
// (fma), then the wave butterfly (lane offsets 32, 16, .., 1).  dl: us[i] <- (us[i] - X[i])·scale (the
// cotangent, formed as native_mse_gradient forms it: a rounded difference, then a rounded product).
template <bool DL>
__device__ __forceinline__ double wave_mse(double* __restrict__ us, const double* __restrict__ X, int64_t cnt,
                                           double scale) {
    const int lane = threadIdx.x & (kWave - 1);
    double s = 0.0;
    for (int64_t i = lane; i < cnt; i += kWave) {
        const double d = __dsub_rn(us[i], X[i]);
        s = ::fma(d, d, s);
        if constexpr (DL) us[i] = __dmul_rn(d, scale);
    }
    return __ddiv_rn(wave_sum(s), (double)cnt);
}

// mse + λ·Σ_q |ps[q]| over the calling wave (reg_loss(p, λ, 0), LV_driver_KANODE.jl:187-201), ps in LDS: the sum in
// wave_mse's order (lane l adds its entries l, l + 64, .. ascending, then the wave butterfly), then one rounded
// product and one rounded sum.  An entry that is exactly zero makes the loss NaN, as the host formula is there
// (its entropy term is 0·log 0 even at weight 0): the loop then stops with kTrainLossNotFinite.
__device__ __forceinline__ double l1_loss(double mse, const double* __restrict__ ps, int P, double lam) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1);
    double s = 0.0;
    bool zero = false;
    for (int q = lane; q < P; q += kWave) {
        const double x = ps[q];
        s = s + ::fabs(x);
        zero = zero || x == 0.0;
    }
    const double A = wave_sum(s);
    const double lv = mse + lam * A;
    return __any(zero) ? __longlong_as_double(0x7ff8000000000000LL) : lv;
}

// NORM: the adjoint's normalizer; FN, PATH, FS: the forward's ChainModel specialisation (what
// launch_kd_chain_tsit5 picks for the handle)
template <int NORM, int FN, int PATH, class FS>
__global__ void __launch_bounds__((kLvSpWaves + 1) * kWave)
kd_chain_train_lvsp_kernel(const LayerConst* __restrict__ lcs, ChainTrainArgs a) {
    constexpr int N = LvWaveShape::I, P = kLvP;
    extern __shared__ __attribute__((aligned(16))) unsigned char cv_raw[];
    LayerConst* lcl = reinterpret_cast<LayerConst*>(cv_raw);
    double* ps = reinterpret_cast<double*>(cv_raw + 2 * sizeof(LayerConst));
    double* tsl = ps + P;            // [cap]
    double* dtsl = tsl + a.cap;      // [cap]
    double* recl = dtsl + a.cap;     // [cap][7][N], then k1_0 [N] (stage_rec)
    double* sv = a.stage_rec ? recl + (a.cap * 7 + 1) * N : recl;   // saveat [n_save]
    double* dl = sv + a.n_save;      // u_save, then dl [n_save][N]
    double* svt = dl + a.n_save * N; // the test problem's saveat [n_save_test]
    double* ust = svt + a.n_save_test;   // its u_save [n_save_test][N]
    __shared__ LvSpLds S;
    __shared__ int64_t fo[2][4];     // the counters of wave 0's and wave 1's solve
    __shared__ double lossv;         // loss[it]
    S.fill_tableau();
    {
        const int nw = 2 * (int)(sizeof(LayerConst) / sizeof(int32_t));
        const int32_t* src = reinterpret_cast<const int32_t*>(lcs);
        int32_t* dst = reinterpret_cast<int32_t*>(cv_raw);
        stage_chain_consts(dst, src, nw, ps, a.p, P);
        for (int64_t i = threadIdx.x; i < a.n_save; i += blockDim.x) sv[i] = a.saveat[i];
        for (int64_t i = threadIdx.x; i < a.n_save_test; i += blockDim.x) svt[i] = a.saveat_test[i];
        if (threadIdx.x < 8) fo[threadIdx.x / 4][threadIdx.x % 4] = 0;
    }
    KAN_EXP_TABLE_LDS(tab);
    const Math<double> M{tab};
    const int lane = threadIdx.x & (kWave - 1);
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const bool has_test = a.n_save_test > 0 && a.loss_test != nullptr;
    double* const rec = a.stage_rec ? recl : a.rec;
    double* const rk1 = rec + a.cap * 7 * N;
    ChainAdjointArgs aa{};   // (rec, k1_0, ts, dts, nsteps and the outputs: lvsp_adjoint's own arguments)
    aa.t0 = a.t0;
    aa.tf = a.tf;
    aa.dt = a.dt;
    aa.abstol = a.abstol;
    aa.reltol = a.reltol;
    aa.dtmin = a.dtmin;
    aa.beta1 = a.beta1;
    aa.beta2 = a.beta2;
    aa.gamma = a.gamma;
    aa.qmin = a.qmin;
    aa.qmax = a.qmax;
    aa.qoldinit = a.qoldinit;
    aa.adaptive = a.adaptive;
    aa.maxiters = a.maxiters;
    aa.dl_du = dl;
    aa.stops = a.stops;
    aa.nstops = a.nstops;
    aa.jrows = a.jrows;
    aa.joff = a.joff;
    double bp1 = a.bp1, bp2 = a.bp2;
    int64_t done = 0;
    int reason = kTrainOk;
    for (int64_t it = 0; it <= a.n_iters; ++it) {
        if (it == a.n_iters && !(has_test && it > 0)) break;
        // ---- A: the solves at p_it (wave 0: training, dense output kept; wave 1: test) ----
        const bool tst = w == 1;
        if (w < 2 && (tst ? (has_test && it > 0) : it < a.n_iters)) {
            ChainSolveArgs fa{};
            fa.t0 = a.t0;
            fa.tf = tst ? a.tf_test : a.tf;
            fa.dt = a.dt;
            fa.abstol = a.abstol;
            fa.reltol = a.reltol;
            fa.dtmin = a.dtmin;
            fa.beta1 = a.beta1;
            fa.beta2 = a.beta2;
            fa.gamma = a.gamma;
            fa.qmin = a.qmin;
            fa.qmax = a.qmax;
            fa.qoldinit = a.qoldinit;
            fa.adaptive = a.adaptive;
            fa.maxiters = a.maxiters;
            fa.n_save = tst ? a.n_save_test : a.n_save;
            fa.cap = a.cap;
            fa.saveat = tst ? svt : sv;
            fa.u_save = tst ? ust : dl;
            fa.rec = tst ? nullptr : rec;
            fa.k1_0 = rk1;
            fa.ts = tsl;
            fa.dts = dtsl;
            fa.out = fo[tst ? 1 : 0];
            const int j = threadIdx.x & (kChainDim - 1);
            ChainModel<double, FN, PATH, FS> fm{M, lcl, 2, ps, nullptr, P, j, 0, lane < N, (int64_t)lane, (int64_t)N};
            onewg_tsit5<double, ChainModel<double, FN, PATH, FS>, true>(fm, a.u0, fa, nullptr);
            __threadfence_block();   // the wave's u_save (lanes < N wrote it) before every lane reads it
            if (tst) {
                const double lt = wave_mse<false>(ust, a.target_test, a.n_save_test * N, 0.0);
                if (lane == 0) a.loss_test[it - 1] = fo[1][3] == 0 ? lt : __longlong_as_double(0x7ff8000000000000LL);
            } else if (fo[0][3] == 0) {   // (lane 0's own store, read back by the wave)
                double lv = wave_mse<true>(dl, a.target, a.n_save * N, a.dl_scale);
                if (a.act_reg != 0.0) lv = l1_loss(lv, ps, P, a.act_reg);   // (λ = 0: not one operation more)
                if (lane == 0) {
                    a.loss[it] = lv;
                    lossv = lv;
                }
            }
        }
        __syncthreads();
        if (has_test && it > 0 && fo[1][3] != 0) {
            reason = kTrainTestMaxiters;
            break;
        }
        if (it == a.n_iters) break;
        if (fo[0][3] != 0) {
            reason = fo[0][3] == 2 ? kTrainDenseCapacity : kTrainForwardMaxiters;
            break;
        }
        if (!(::fabs(lossv) <= 1.7976931348623157e308)) {
            reason = kTrainLossNotFinite;
            break;
        }
        // ---- B: the InterpolatingAdjoint from the dense output just written ----
        double mu[kLvPL], l0, l1;
        int64_t res[4];
        lvsp_adjoint<NORM>(S, M, lcl, ps, aa, fo[0][0], rec, rk1, tsl, dtsl, mu, l0, l1, res);
        if (res[3] != 0) {
            reason = kTrainAdjointMaxiters;
            break;
        }
        // ---- C: records and Adam (wave 0: lane l holds the gradient entries l + 64 r) ----
        if (w == 0) {
            if (a.counts && lane == 0) {
                a.counts[4 * it] = fo[0][0];
                a.counts[4 * it + 1] = fo[0][1];
                a.counts[4 * it + 2] = res[0];
                a.counts[4 * it + 3] = res[1];
            }
            AdamArgs ad;
            ad.scale = 1.0;
            ad.beta1 = a.ab1;
            ad.beta2 = a.ab2;
            ad.omb1 = a.omb1;
            ad.omb2 = a.omb2;
            {   // (contraction off: 1 - βp must not fuse with the product that advanced βp below)
#pragma clang fp contract(off)
                ad.c1 = 1.0 - bp1;
                ad.c2 = 1.0 - bp2;
            }
            ad.eps = a.eps;
            ad.eta = a.eta;
#pragma unroll
            for (int r = 0; r < kLvPL; ++r) {
                const int q = lane + kWave * r;
                if (q < P) {
                    const double x = ps[q];
                    double gq = mu[r];
                    // ∂(λ·Σ|p|)/∂p_q = λ·sgn(p_q), sgn(0) = 0: one rounded add (λ = 0: none, a -0.0 stays -0.0)
                    if (a.act_reg != 0.0) gq = __dadd_rn(gq, x > 0.0 ? a.act_reg : (x < 0.0 ? -a.act_reg : 0.0));
                    if (a.grad) a.grad[it * P + q] = gq;
                    if (a.p_before) a.p_before[it * P + q] = x;
                    double mq = a.m[q], vq = a.v[q];
                    const double xn = adam_entry<double>(x, mq, vq, gq, ad);
                    a.m[q] = mq;
                    a.v[q] = vq;
                    a.p[q] = xn;
                    ps[q] = xn;
                }
            }
        }
        __syncthreads();   // p_{it+1} in LDS; every wave is done with dl, the dense output and the rows
        {   // the rounded products Python's `bp *= β` forms
#pragma clang fp contract(off)
            bp1 = bp1 * a.ab1;
            bp2 = bp2 * a.ab2;
        }
        done = it + 1;
    }
    if (threadIdx.x == 0) {
        a.out[0] = done;
        a.out[1] = reason;
    }
}

bool chain_train_supported(const LayerConst* hlcs, int nl, int64_t P, int64_t B, size_t esize, bool wide) {
    // (one path specialisation for both layers: launch_kd_chain_tsit5's condition, whose arithmetic the forward is)
    return KAN_LV_SP && esize == sizeof(double) && P == kLvP && chain_is_lv_wave(hlcs, nl, B, wide) &&
           hlcs[0].path == hlcs[1].path;
}

size_t chain_train_lds(int64_t cap, int64_t n_save, int64_t n_save_test, int* stage_rec) {
    constexpr size_t kBudget = 140 * 1024;   // launch_kd_chain_adjoint's, with cap in place of nsteps
    const size_t jst = sizeof(double) * 8 * LvWaveShape::I * (kLvP + LvWaveShape::I);
    const size_t rec = sizeof(double) * ((size_t)cap * 7 + 1) * LvWaveShape::I;
    size_t lsp = 2 * sizeof(LayerConst) +
                 sizeof(double) * (kLvP + 2 * (size_t)cap + (size_t)(1 + LvWaveShape::I) * (n_save + n_save_test));
    const int sr = lsp + rec + jst <= kBudget ? 1 : 0;
    if (sr) lsp += rec;
    if (stage_rec) *stage_rec = sr;
    return lsp + jst <= kBudget ? lsp : 0;
}

hipError_t launch_kd_chain_train(const LayerConst* hlcs, int nl, const LayerConst* lcs, int64_t P,
                                 const ChainTrainArgs& a, hipStream_t st) {
    if (!chain_train_supported(hlcs, nl, P, 1, sizeof(double), true) || a.cap < 1 || a.cap > kChainAdjointMaxSteps ||
        a.n_iters < 1 || a.n_save < 0 || a.n_save_test < 0)
        return hipErrorNotSupported;
    int sr = 0;
    const size_t lds = chain_train_lds(a.cap, a.n_save, a.n_save_test, &sr);
    if (lds == 0 || sr != a.stage_rec || (!sr && !a.rec)) return hipErrorNotSupported;
    const LayerConst& h = hlcs[0];
    const bool tf = h.norm == NORM_TANH_FAST;
    // the forward's specialisation: launch_kd_chain_tsit5's choice for this handle
#define KAN_TRAIN_GO(NORM, FN, PATH, FS)                                                                            \
    do {                                                                                                            \
        const void* fn = reinterpret_cast<const void*>(&kd_chain_train_lvsp_kernel<NORM, FN, PATH, FS>);            \
        const hipError_t e = ensure_dynamic_lds(fn, lds);                                                           \
        if (e != hipSuccess) return e;                                                                              \
        hipLaunchKernelGGL((kd_chain_train_lvsp_kernel<NORM, FN, PATH, FS>), dim3(1),                               \
                           dim3((kLvSpWaves + 1) * kWave), lds, st, lcs, a);                                        \
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

}  // namespace kan
