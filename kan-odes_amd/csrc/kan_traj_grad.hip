// kan_traj_grad.hip — the gradient of a trajectory ensemble in one launch (gfx950): R initial conditions of ONE small
// chain at ONE parameter vector, every trajectory an ODE of its own (its own error norm, step sizes, rejections and
// adjoint steps), the loss mean((u - X)²) over the whole [n_save][R][N] tensor and its gradient, the mean of the R
// batch-1 gradients (kanode_trajectories_gradient_tsit5).  kan_traj_solve.hip is the forward-only entry of the same
// reading; kd_chain_train_wg_kernel at a batch is the other one (ONE ODE over all B·N entries).
//
// kd_chain_traj_grad_kernel: one one-wave workgroup per trajectory, a grid of the launch group's size.  Workgroup r
// runs phases A and B of kan_train_wg_body.inc exactly once at B = 1, by the same functions (kan_train_wg_phases.hpp):
//   A  wg_forward: onewg_tsit5 in block mode on ChainModel from u0[r]; the dense output goes to the trajectory's
//      private global block, ts / dts stay in LDS, u_save stays in LDS where it fits (dl_lds).  barrier.  The u_save
//      columns go out (optional), then wg_loss: mse_r = wave_mse<true> against the trajectory's target rows, which
//      the workgroup first gathered from target[:, r, :] into its private block (wave_mse reads one dense array).
//   B  onewg_adjoint on ChainModel, always (the column-group model on one wave: chain_adjoint_plan at B = 1 with
//      wide = false).  One wave per trajectory is the throughput layout at R in the hundreds; the [2,10,2] chain runs
//      here on the ChainShapeLV rung.
// Then the workgroup writes its row [P + 1] (the gradient, mse_r in column P), the optional copies and its eight
// status words.  A trajectory that stops (ChainTrainStop) stops alone: its status is written, its row is NaN.  No
// workgroup reads what another writes; no grid barrier, no spin; every barrier is reached by the whole one-wave block
// (the stop decisions read LDS words behind a barrier, so they are uniform).
//
// traj_grad_chunk_kernel / traj_grad_total_kernel: dp[q] = (Σ_r rows[r][q]) / R in an order that is a function of R
// alone: chunks of 64 consecutive trajectories summed in ascending r from 0.0 with rounded adds, the chunk sums then
// summed in ascending chunk order from 0.0, one rounded division by R.  Column P gives the loss.  No atomics.
#define KAN_COL_DEVICE_ONLY
#include "kan_col.hip"
#include "kan_ensemble.hpp"
#include "kan_train_loss.hpp"
#include "kan_train_wg_phases.hpp"

namespace kan {

namespace {

// B with dL/du0 written (a function of its own, as wg_adjoint is; du0 may be null)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wpass-failed"
template <int FN, int PATH, class FS>
__device__ __noinline__ void traj_adjoint(const ChainTrainArgs& a, const TrainWgPtrs& L, double* du0) {
    constexpr int ADJ = kWgChain, WN = NORM_RUNTIME;
#define KAN_WG_ADJOINT_DU0 aa.du0 = wg_uniform(du0);
#include "kan_train_wg_adjoint.inc"
#undef KAN_WG_ADJOINT_DU0
}
#pragma clang diagnostic pop

template <int FN, int PATH, class FS>
__global__ void __launch_bounds__(kWave)
kd_chain_traj_grad_kernel(const LayerConst* __restrict__ lcs, int nl, int P, TrajGradArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tg_raw[];
    __shared__ double red[1];
    __shared__ int64_t fo[12];
    __shared__ double lossv;
    const int64_t r = blockIdx.x;
    const int64_t n = g.t.N;   // (B = 1)
    double* const blk = reinterpret_cast<double*>(g.blocks + (size_t)r * g.block_stride);
    double* const row = g.rows + (size_t)r * traj_grad_row_elems(P);
    ChainTrainArgs a = g.t;
    a.u0 = g.u0 + traj_grad_u0_elem(r, n, 0);
    a.rec = blk;
    a.target = blk + traj_grad_block_target(n, a.cap, a.n_save);
    a.loss = row + P;
    const int64_t work = (int64_t)(blockDim.x / kChainDim) * P;
    const TrainWgCarve c = train_wg_carve(P, work, a.cap, a.n_save, 0, n, a.dl_lds, 0);
    double* const base = reinterpret_cast<double*>(tg_raw + nl * sizeof(LayerConst));
    TrainWgPtrs L;
    L.lcl = (KAN_LDS const LayerConst*)reinterpret_cast<const LayerConst*>(tg_raw);
    L.ps = (KAN_LDS double*)(base + c.ps);
    L.work = (KAN_LDS double*)(base + c.work);
    L.mu = (KAN_LDS double*)(base + c.mu);
    L.km = (KAN_LDS double*)(base + c.km);
    L.gl = (KAN_LDS double*)(base + c.gl);
    L.tsl = (KAN_LDS double*)(base + c.tsl);
    L.dtsl = (KAN_LDS double*)(base + c.dtsl);
    L.sv = (KAN_LDS double*)(base + c.sv);
    L.svt = (KAN_LDS double*)(base + c.svt);
    L.rec = a.rec;
    L.rk1 = a.rec + a.cap * 7 * n;
    L.dl = a.dl_lds ? base + c.dl : blk + traj_grad_block_usave(n, a.cap);
    L.ust = nullptr;
    L.recl = (KAN_LDS double*)(base + c.recl);
    L.red = (KAN_LDS double*)red;
    L.fo = (KAN_LDS int64_t*)fo;
    L.lossv = (KAN_LDS double*)&lossv;
    L.nl = nl;
    L.P = P;
    {
        const int nw = nl * (int)(sizeof(LayerConst) / sizeof(int32_t));
        const int32_t* src = reinterpret_cast<const int32_t*>(lcs);
        int32_t* dst = reinterpret_cast<int32_t*>(tg_raw);
        stage_chain_consts(dst, src, nw, base + c.ps, a.p, P);
        for (int64_t i = threadIdx.x; i < a.n_save; i += blockDim.x) L.sv[i] = a.saveat[i];
        // target[:, r, :] as one dense [n_save][n] array in the private block
        double* const tg = blk + traj_grad_block_target(n, a.cap, a.n_save);
        for (int64_t i = threadIdx.x; i < a.n_save * n; i += blockDim.x)
            tg[i] = g.target[traj_grad_save_elem(i / n, r, g.R_all, n, i % n)];
        if (threadIdx.x < 12) fo[threadIdx.x] = 0;
    }
    KAN_EXP_TABLE_LDS(tab);   // (its barrier also publishes the constants, ps, the saveat list, the target rows and fo)
    L.tab = (KAN_LDS const double*)tab;
    int reason = kTrainOk;
    // ---- A: the solve, the loss and its cotangent ----
    wg_forward<FN, PATH, FS>(a, L, false);
    __syncthreads();   // u_save, the dense output, ts / dts and the counters
    if (fo[3] == 0) {
        if (g.u_save)
            for (int64_t i = threadIdx.x; i < a.n_save * n; i += blockDim.x)
                g.u_save[traj_grad_save_elem(i / n, r, g.R_all, n, i % n)] = L.dl[i];
        __syncthreads();   // (before wg_loss turns u_save into the cotangent)
        wg_loss(a, L, 0);
    }
    __syncthreads();
    if (fo[3] != 0) reason = fo[3] == 2 ? kTrainDenseCapacity : kTrainForwardMaxiters;
    else if (!(::fabs(lossv) <= 1.7976931348623157e308)) reason = kTrainLossNotFinite;
    // ---- B: the InterpolatingAdjoint from the dense output just written ----
    if (reason == kTrainOk) {
        traj_adjoint<FN, PATH, FS>(a, L, g.du0 ? g.du0 + traj_grad_u0_elem(r, n, 0) : nullptr);
        __syncthreads();   // the gradient and the adjoint's counters
        if (fo[11] != 0) reason = kTrainAdjointMaxiters;
    }
    // ---- the row, the optional copies, the status words ----
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int q = threadIdx.x; q < P; q += blockDim.x) {
        const double v = reason == kTrainOk ? L.gl[q] : nan;
        row[q] = v;
        if (g.dp_rows) g.dp_rows[(size_t)r * P + q] = v;
    }
    if (reason != kTrainOk && g.du0)
        for (int64_t i = threadIdx.x; i < n; i += blockDim.x) g.du0[traj_grad_u0_elem(r, n, i)] = nan;
    if (threadIdx.x == 0) {
        const double lv = reason == kTrainOk ? lossv : nan;
        row[P] = lv;
        if (g.loss_rows) g.loss_rows[r] = lv;
        int64_t* const w = g.status + traj_grad_status_word(r);
        for (int i = 0; i < 4; ++i) {
            w[i] = fo[i];
            w[4 + i] = fo[8 + i];
        }
        if (reason == kTrainLossNotFinite) w[7] = kTrajGradAdjointSkipped;
    }
}

// part[c][q] = rows[64 c][q] + .. + rows[min(R, 64 c + 64) - 1][q], from 0.0 in ascending r, rounded adds
__global__ void __launch_bounds__(kBlock)
traj_grad_chunk_kernel(const double* __restrict__ rows, int64_t R, int W, double* __restrict__ part) {
    const int q = blockIdx.y * kBlock + threadIdx.x;
    if (q >= W) return;
    const int64_t c = blockIdx.x, r1 = traj_grad_chunk_end(c, R);
    double s = 0.0;
    for (int64_t r = traj_grad_chunk_begin(c); r < r1; ++r) s = __dadd_rn(s, rows[(size_t)r * W + q]);
    part[(size_t)c * W + q] = s;
}
// out[q] = (part[0][q] + .. + part[nchunk - 1][q]) / R, from 0.0 in ascending chunk order; q < W - 1 -> dp, the
// last column -> *loss
__global__ void __launch_bounds__(kBlock)
traj_grad_total_kernel(const double* __restrict__ part, int64_t nchunk, int64_t R, int W, double* __restrict__ dp,
                       double* __restrict__ loss) {
    const int q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= W) return;
    double s = 0.0;
    for (int64_t c = 0; c < nchunk; ++c) s = __dadd_rn(s, part[(size_t)c * W + q]);
    const double v = __ddiv_rn(s, (double)R);
    if (q < W - 1) dp[q] = v;
    else *loss = v;
}

}  // namespace

bool chain_traj_grad_supported(const LayerConst* hlcs, int nl, int64_t P, size_t esize) {
    return chain_train_wg_supported(hlcs, nl, P, 1, esize, false);
}

size_t chain_traj_grad_lds(const LayerConst* hlcs, int nl, int64_t P, int64_t cap, int64_t n_save, int* dl_lds) {
    int sr = 0;
    return chain_train_wg_lds(hlcs, nl, P, 1, false, cap, n_save, 0, dl_lds, &sr);
}

hipError_t launch_kd_chain_traj_grad(const LayerConst* hlcs, int nl, const LayerConst* lcs, int64_t P,
                                     const TrajGradArgs& g, int64_t R, hipStream_t st) {
    const ChainTrainArgs& a = g.t;
    if (!chain_traj_grad_supported(hlcs, nl, P, sizeof(double)) || R < 1 || R > kTrajMaxTrajectories || a.B != 1 ||
        a.N != hlcs[0].I || a.n_save < 1 || a.n_save_test != 0 || a.stage_rec != 0 || !a.p || !g.u0 || !g.target ||
        !g.blocks || !g.rows || !g.status || g.R_all < R ||
        g.block_stride < sizeof(double) * traj_grad_block_elems(a.N, a.cap, a.n_save))
        return hipErrorNotSupported;
    int dl = 0;
    const size_t lds = chain_traj_grad_lds(hlcs, nl, P, a.cap, a.n_save, &dl);
    if (lds == 0 || dl != a.dl_lds) return hipErrorNotSupported;
    // the column-group adjoint on one wave, whatever the handle's chain_wide says
    const ChainAdjPlan plan = chain_adjoint_plan(kChainLimits, hlcs, nl, P, 1, false, a.cap, sizeof(double), false);
    if (plan.model != kAdjChain || plan.threads != kWave) return hipErrorNotSupported;
    return chain_ladder(hlcs, nl, [&](auto norm, auto path, auto shape) {
        const void* fn = reinterpret_cast<const void*>(&kd_chain_traj_grad_kernel<norm(), path(), decltype(shape)>);
        const hipError_t e = ensure_dynamic_lds(fn, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((kd_chain_traj_grad_kernel<norm(), path(), decltype(shape)>), dim3((unsigned)R),
                           dim3(kWave), lds, st, lcs, nl, (int)P, g);
        return hipGetLastError();
    });
}

hipError_t launch_traj_grad_chunks(const double* rows, int64_t R, int64_t P, double* part, hipStream_t st) {
    if (R < 1 || R > kTrajMaxTrajectories || P < 1 || !rows || !part) return hipErrorInvalidValue;
    const int W = (int)traj_grad_row_elems(P);
    const dim3 grid((unsigned)traj_grad_chunks(R), (unsigned)((W + kBlock - 1) / kBlock));
    hipLaunchKernelGGL(traj_grad_chunk_kernel, grid, dim3(kBlock), 0, st, rows, R, W, part);
    return hipGetLastError();
}

hipError_t launch_traj_grad_total(const double* part, int64_t R, int64_t P, double* dp, double* loss, hipStream_t st) {
    if (R < 1 || R > kTrajMaxTrajectories || P < 1 || !part || !dp || !loss) return hipErrorInvalidValue;
    const int W = (int)traj_grad_row_elems(P);
    hipLaunchKernelGGL(traj_grad_total_kernel, dim3((unsigned)((W + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, part,
                       traj_grad_chunks(R), R, W, dp, loss);
    return hipGetLastError();
}

#undef KAN_LDS

}  // namespace kan
