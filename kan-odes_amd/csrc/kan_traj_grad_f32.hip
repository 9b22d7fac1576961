// kan_traj_grad_f32.hip — the gradient of a trajectory ensemble in fp32, one launch (gfx950): kan_traj_grad.hip's
// problem for a small fp32 chain (kanode_trajectories_gradient_f32_tsit5).  R initial conditions of ONE chain at ONE
// float parameter vector, every trajectory an ODE of its own, the loss mean((u - X)²) over the whole [n_save][R][N]
// tensor and its gradient, the mean of the R batch-1 gradients.
//
// kd_chain_traj_grad_f32_kernel: one one-wave workgroup per trajectory, a grid of the launch group's size.  Workgroup r
//   staging  the layer constants and p (float) into LDS, the saveat list (double); the group rows, μ and kμ zeroed as
//            kd_chain_adjoint_kernel zeroes them; the eight counters zeroed.  (No exp table: Math<float> reads none.)
//   forward  onewg_tsit5<float> in block mode on ChainModel<float, ..> from u0[r] at B = 1 with the argument values
//            kd_chain_tsit5_kernel<float> gets; the dense output [cap][7][N] and k1_0 go as float to the trajectory's
//            private global block, ts / dts stay double in LDS, u_save is float in LDS where it fits (dl_lds), else in
//            the block.
//   loss     d = u - X (a rounded float difference, X read from target[:, r, :] by index), the cotangent
//            d · (float)(2 / (n_save·N)) in place of u_save (a rounded float product: what (u_save - target).mul_(2.0 /
//            numel) computes on a float tensor), mse_r = Σ (double)d² / (n_save·N) summed in double on the wave (lane l
//            its terms l, l + 64, .. by fma, then the butterfly) and rounded to float once.
//   adjoint  onewg_adjoint<float> on ChainModel<float, ..> with the column-group rows, always (chain_adjoint_plan at
//            B = 1 with wide = false gives kAdjChain on 64 threads); dL/du0 goes out.
// Then the row [P + 1] floats (the gradient, mse_r in column P), the optional copies and the eight status words of
// kan_traj_grad.hip.  A trajectory that stops (ChainTrainStop) stops alone: its row, mse_r and du0 are NaN.  No
// workgroup reads what another writes; no grid barrier, no spin, no atomics; the stop decisions read LDS words behind
// a barrier, so every barrier is reached by the whole one-wave block.
//
// The phases are plain inlined code here (the fp64 kernel calls its phases as functions of their own and moves their
// arguments to scalar registers by hand): every argument is a kernel argument, so the compiler already holds the
// solver options in scalar registers, and a float instantiation needs half the registers of a double one.
//
// traj_grad_chunk_f32_kernel / traj_grad_total_f32_kernel: kan_traj_grad.hip's reduction on float rows, the same order
// (kan_ensemble.hpp's chunks) with __fadd_rn and one __fdiv_rn by (float)R (R <= 65536 is exact in float): bit for bit
// kanode.adjoint.combine_trajectory_rows on float32 rows.
#define KAN_COL_DEVICE_ONLY
#include "kan_col.hip"
#include "kan_ensemble.hpp"

namespace kan {

namespace {

// (the generic shapes are too large for the stage loops to be unrolled, as in kan_col.hip's adjoint kernels)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wpass-failed"
template <int FN, int PATH, class FS>
__global__ void __launch_bounds__(kWave)
kd_chain_traj_grad_f32_kernel(const LayerConst* __restrict__ lcs, int nl, int P, TrajGradF32Args g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tgf_raw[];
    __shared__ double red[1];
    __shared__ int64_t fo[kTrajGradStatusWords];   // the forward's four counters, then the adjoint's
    __shared__ float lossv;
    const int64_t r = blockIdx.x;
    const ChainTrainArgs& a = g.t;
    const int N = (int)a.N;   // (B = 1)
    const int64_t n = N, cnt = a.n_save * n;
    float* const blk = reinterpret_cast<float*>(g.blocks + (size_t)r * g.block_stride);
    float* const row = g.rows + (size_t)r * traj_grad_row_elems(P);
    constexpr int NG = kWave / kChainDim;
    const TrajGradF32Carve c = traj_grad_f32_carve(P, NG, a.cap, a.n_save, n, a.dl_lds);
    unsigned char* const base = tgf_raw + nl * sizeof(LayerConst);
    const LayerConst* const lcl = reinterpret_cast<const LayerConst*>(tgf_raw);
    float* const ps = reinterpret_cast<float*>(base + c.ps);
    float* const work = reinterpret_cast<float*>(base + c.work);   // [NG][P] group rows | μ [2][P] | kμ [7][P]
    float* const mu = reinterpret_cast<float*>(base + c.mu);
    float* const km = reinterpret_cast<float*>(base + c.km);
    float* const gl = reinterpret_cast<float*>(base + c.gl);
    double* const tsl = reinterpret_cast<double*>(base + c.tsl);
    double* const dtsl = reinterpret_cast<double*>(base + c.dtsl);
    double* const sv = reinterpret_cast<double*>(base + c.sv);
    float* const rec = blk;
    float* const rk1 = blk + a.cap * 7 * n;
    float* const dl = a.dl_lds ? reinterpret_cast<float*>(base + c.dl) : blk + traj_grad_f32_block_usave(n, a.cap);
    {
        const int nw = nl * (int)(sizeof(LayerConst) / sizeof(int32_t));
        const int32_t* src = reinterpret_cast<const int32_t*>(lcs);
        int32_t* dst = reinterpret_cast<int32_t*>(tgf_raw);
        stage_chain_consts(dst, src, nw, ps, g.p, P);
        for (int i = threadIdx.x; i < NG * P + 9 * P; i += blockDim.x) work[i] = 0.0f;
        for (int64_t i = threadIdx.x; i < a.n_save; i += blockDim.x) sv[i] = a.saveat[i];
        if (threadIdx.x < kTrajGradStatusWords) fo[threadIdx.x] = 0;
    }
    __syncthreads();   // the constants, ps, the zeroed rows, the saveat list and fo
    const Math<float> M{nullptr};
    const int j = threadIdx.x & (kChainDim - 1);
    const int64_t col = threadIdx.x / kChainDim;
    const bool act = col < 1 && j < N;
    int reason = kTrainOk;
    // ---- the solve ----
    {
        ChainSolveArgs fa{};
        fa.t0 = a.t0, fa.tf = a.tf, fa.dt = a.dt, fa.abstol = a.abstol, fa.reltol = a.reltol, fa.dtmin = a.dtmin;
        fa.beta1 = a.beta1, fa.beta2 = a.beta2, fa.gamma = a.gamma, fa.qmin = a.qmin, fa.qmax = a.qmax;
        fa.qoldinit = a.qoldinit;
        fa.adaptive = a.adaptive;
        fa.maxiters = a.maxiters;
        fa.n_save = a.n_save;
        fa.cap = a.cap;
        fa.saveat = sv;
        fa.u_save = dl;
        fa.rec = rec;
        fa.k1_0 = rk1;
        fa.ts = tsl;
        fa.dts = dtsl;
        fa.out = fo;
        ChainModel<float, FN, PATH, FS> m{M, lcl, nl, ps, nullptr, P, j, 0, act, (int64_t)N * col + j, n};
        onewg_tsit5<float>(m, g.u0 + traj_grad_u0_elem(r, n, 0), fa, red);
    }
    __syncthreads();   // u_save, the dense output, ts / dts and the counters
    // ---- the loss and its cotangent ----
    if (fo[3] == 0) {
        if (g.u_save)
            for (int64_t i = threadIdx.x; i < cnt; i += blockDim.x)
                g.u_save[traj_grad_save_elem(i / n, r, g.R_all, n, i % n)] = dl[i];
        const float scale = (float)a.dl_scale;
        double s = 0.0;
        for (int64_t i = threadIdx.x; i < cnt; i += kWave) {   // (each lane turns only entries it read itself)
            const float d = __fsub_rn(dl[i], g.target[traj_grad_save_elem(i / n, r, g.R_all, n, i % n)]);
            s = ::fma((double)d, (double)d, s);
            dl[i] = __fmul_rn(d, scale);
        }
        const float lv = (float)__ddiv_rn(wave_sum(s), (double)cnt);
        if (threadIdx.x == 0) lossv = lv;
    }
    __syncthreads();   // the cotangent and lossv
    if (fo[3] != 0) reason = fo[3] == 2 ? kTrainDenseCapacity : kTrainForwardMaxiters;
    else if (!(::fabsf(lossv) <= 3.402823466e+38f)) reason = kTrainLossNotFinite;
    // ---- the InterpolatingAdjoint from the dense output just written ----
    if (reason == kTrainOk) {
        ChainAdjointArgs aa{};
        aa.t0 = a.t0, aa.tf = a.tf, aa.dt = a.dt, aa.abstol = a.abstol, aa.reltol = a.reltol, aa.dtmin = a.dtmin;
        aa.beta1 = a.beta1, aa.beta2 = a.beta2, aa.gamma = a.gamma, aa.qmin = a.qmin, aa.qmax = a.qmax;
        aa.qoldinit = a.qoldinit;
        aa.adaptive = a.adaptive;
        aa.maxiters = a.maxiters;
        aa.rec = rec;
        aa.k1_0 = rk1;
        aa.ts = tsl;
        aa.dts = dtsl;
        aa.nsteps = fo[0];
        aa.dl_du = dl;
        aa.stops = a.stops;
        aa.nstops = a.nstops;
        aa.jrows = a.jrows;
        aa.joff = a.joff;
        aa.du0 = g.du0 ? g.du0 + traj_grad_u0_elem(r, n, 0) : nullptr;
        aa.dp = gl;
        aa.out = fo + 4;
        ChainModel<float, FN, PATH, FS> m{M, lcl, nl, ps, work, P, j, 1, act, (int64_t)N * col + j, n};
        onewg_adjoint<float>(m, aa, mu, km, tsl, dtsl, red);
        __syncthreads();   // the gradient and the adjoint's counters
        if (fo[7] != 0) reason = kTrainAdjointMaxiters;
    }
    // ---- the row, the optional copies, the status words ----
    const float nan = __int_as_float(0x7fc00000);
    for (int q = threadIdx.x; q < P; q += blockDim.x) {
        const float v = reason == kTrainOk ? gl[q] : nan;
        row[q] = v;
        if (g.dp_rows) g.dp_rows[(size_t)r * P + q] = v;
    }
    if (reason != kTrainOk && g.du0)
        for (int64_t i = threadIdx.x; i < n; i += blockDim.x) g.du0[traj_grad_u0_elem(r, n, i)] = nan;
    if (threadIdx.x == 0) {
        const float lv = reason == kTrainOk ? lossv : nan;
        row[P] = lv;
        if (g.loss_rows) g.loss_rows[r] = lv;
        int64_t* const w = g.status + traj_grad_status_word(r);
        for (int i = 0; i < kTrajGradStatusWords; ++i) w[i] = fo[i];
        if (reason == kTrainLossNotFinite) w[7] = kTrajGradAdjointSkipped;
    }
}
#pragma clang diagnostic pop

// part[c][q] = rows[64 c][q] + .. + rows[min(R, 64 c + 64) - 1][q], from 0.0f in ascending r, rounded adds
__global__ void __launch_bounds__(kBlock)
traj_grad_chunk_f32_kernel(const float* __restrict__ rows, int64_t R, int W, float* __restrict__ part) {
    const int q = blockIdx.y * kBlock + threadIdx.x;
    if (q >= W) return;
    const int64_t c = blockIdx.x, r1 = traj_grad_chunk_end(c, R);
    float s = 0.0f;
    for (int64_t r = traj_grad_chunk_begin(c); r < r1; ++r) s = __fadd_rn(s, rows[(size_t)r * W + q]);
    part[(size_t)c * W + q] = s;
}
// out[q] = (part[0][q] + .. + part[nchunk - 1][q]) / R, from 0.0f in ascending chunk order; q < W - 1 -> dp, the
// last column -> *loss
__global__ void __launch_bounds__(kBlock)
traj_grad_total_f32_kernel(const float* __restrict__ part, int64_t nchunk, int64_t R, int W, float* __restrict__ dp,
                           float* __restrict__ loss) {
    const int q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= W) return;
    float s = 0.0f;
    for (int64_t c = 0; c < nchunk; ++c) s = __fadd_rn(s, part[(size_t)c * W + q]);
    const float v = __fdiv_rn(s, (float)R);
    if (q < W - 1) dp[q] = v;
    else *loss = v;
}

}  // namespace

size_t chain_traj_grad_f32_lds(const LayerConst* hlcs, int nl, int64_t P, int64_t cap, int64_t n_save, int* dl_lds) {
    return traj_grad_f32_lds(kChainLimits, hlcs, nl, P, cap, n_save, dl_lds);
}

bool chain_traj_grad_f32_supported(const LayerConst* hlcs, int nl, int64_t P) {
    return nl >= 1 && chain_tsit5_shape(kChainLimits, hlcs, nl, P, 1, sizeof(float)) &&
           chain_traj_grad_f32_lds(hlcs, nl, P, 1, 1, nullptr) != 0;
}

hipError_t launch_kd_chain_traj_grad_f32(const LayerConst* hlcs, int nl, const LayerConst* lcs, int64_t P,
                                         const TrajGradF32Args& g, int64_t R, hipStream_t st) {
    const ChainTrainArgs& a = g.t;
    if (!chain_traj_grad_f32_supported(hlcs, nl, P) || R < 1 || R > kTrajMaxTrajectories || a.B != 1 ||
        a.N != hlcs[0].I || a.n_save < 1 || a.cap < 1 || !g.p || !g.u0 || !g.target || !g.blocks || !g.rows ||
        !g.status || !a.saveat || !a.stops || !a.jrows || !a.joff || g.R_all < R ||
        g.block_stride < sizeof(float) * traj_grad_f32_block_elems(a.N, a.cap, a.n_save))
        return hipErrorNotSupported;
    int dl = 0;
    const size_t lds = chain_traj_grad_f32_lds(hlcs, nl, P, a.cap, a.n_save, &dl);
    if (lds == 0 || dl != a.dl_lds) return hipErrorNotSupported;
    return chain_ladder(hlcs, nl, [&](auto norm, auto path, auto shape) {
        const void* fn = reinterpret_cast<const void*>(&kd_chain_traj_grad_f32_kernel<norm(), path(), decltype(shape)>);
        const hipError_t e = ensure_dynamic_lds(fn, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((kd_chain_traj_grad_f32_kernel<norm(), path(), decltype(shape)>), dim3((unsigned)R),
                           dim3(kWave), lds, st, lcs, nl, (int)P, g);
        return hipGetLastError();
    });
}

hipError_t launch_traj_grad_chunks_f32(const float* rows, int64_t R, int64_t P, float* part, hipStream_t st) {
    if (R < 1 || R > kTrajMaxTrajectories || P < 1 || !rows || !part) return hipErrorInvalidValue;
    const int W = (int)traj_grad_row_elems(P);
    const dim3 grid((unsigned)traj_grad_chunks(R), (unsigned)((W + kBlock - 1) / kBlock));
    hipLaunchKernelGGL(traj_grad_chunk_f32_kernel, grid, dim3(kBlock), 0, st, rows, R, W, part);
    return hipGetLastError();
}

hipError_t launch_traj_grad_total_f32(const float* part, int64_t R, int64_t P, float* dp, float* loss, hipStream_t st) {
    if (R < 1 || R > kTrajMaxTrajectories || P < 1 || !part || !dp || !loss) return hipErrorInvalidValue;
    const int W = (int)traj_grad_row_elems(P);
    hipLaunchKernelGGL(traj_grad_total_f32_kernel, dim3((unsigned)((W + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                       part, traj_grad_chunks(R), R, W, dp, loss);
    return hipGetLastError();
}

}  // namespace kan
