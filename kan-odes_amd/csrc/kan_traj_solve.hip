// kan_traj_solve.hip — R forward solves of ONE small chain at ONE parameter vector from R initial conditions in one
// launch (gfx950), every trajectory an ODE of its own with its own step control: SciML's EnsembleProblem over u0.
// (kd_chain_tsit5_kernel at a batch is the other reading: ONE ODE over all B·N entries, one error norm, one step
// size; kan_ens_solve.hip varies p and spends a workgroup per replica.)
//
// chain_forward is local to a 16-lane row (DPP row operations, no LDS round trip, no barrier), so a row can carry a
// whole problem: column group g of a block takes trajectory r = blockIdx.x·(blockDim.x / 16) + g and runs
// onewg_tsit5 in its ROW mode (kan_onewg.hpp) — the text the batch-1 solve runs, with the error norm summed over
// the row in the batch-1 kernel's order, so trajectory r has the bits of kd_chain_tsit5_kernel at u0[r] alone.  Lane
// j < N holds u_j and the seven stage values; t, dt, qold, si and the counters are the row's own.
//
// The rows of a wave reject, save and finish at different times, each within maxiters iterations.  After the staging
// barrier (KAN_EXP_TABLE_LDS) NO barrier is executed and no LDS is written: a barrier inside a loop that rows and waves
// leave at different times is the one way this kernel could hang.  With kTrajBlock = 64 (one wave, four trajectories)
// that is structural: the block has no second wave to wait for.  No workgroup reads what another writes; no spin.
// Rows with r >= R leave right after the staging barrier (a partly filled last wave); lanes j >= N of a live row run
// with their row (the DPP sums need them) and store nothing.
#define KAN_COL_DEVICE_ONLY
#include "kan_col.hip"

namespace kan {

namespace {

constexpr int kTrajBlock = kWave;                     // one wave per workgroup
constexpr int kTrajPerBlock = kTrajBlock / kChainDim; // four trajectories

// The small-chain right-hand side of one row: ChainModel's rhs with the row's own entry count beside the stride of
// the saveat rows (onewg_tsit5's ROW mode reads nrow for the norm, n for u_save alone)
template <typename T, int NORM, int PATH, class S>
struct ChainRowModel {
    const Math<T>& M;
    const LayerConst* lcl;
    int nl;
    const T* ps;
    int P, j, nrow;
    bool act;
    int64_t idx, n;
    __device__ T rhs(T y) { return chain_forward<T, NORM, PATH, S>(M, lcl, nl, ps, j, y); }
};

template <typename T, int NORM, int PATH, class S>
__global__ void __launch_bounds__(kTrajBlock)
kd_chain_tsit5_traj_kernel(const LayerConst* __restrict__ lcs, int nl, const T* __restrict__ p, int P,
                           const T* __restrict__ u0, int64_t R, ChainSolveArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cs_raw[];
    LayerConst* lcl = reinterpret_cast<LayerConst*>(cs_raw);
    T* ps = reinterpret_cast<T*>(cs_raw + nl * sizeof(LayerConst));
    {
        const int nw = nl * (int)(sizeof(LayerConst) / sizeof(int32_t));
        const int32_t* src = reinterpret_cast<const int32_t*>(lcs);
        int32_t* dst = reinterpret_cast<int32_t*>(cs_raw);
        stage_chain_consts(dst, src, nw, ps, p, P);
    }
    KAN_EXP_TABLE_LDS(tab);   // the kernel's only barrier (it also publishes lcl, ps)
    const Math<T> M{tab};
    const int N = lcl[0].I;
    const int j = threadIdx.x & (kChainDim - 1);
    const int64_t r = (int64_t)blockIdx.x * (blockDim.x / kChainDim) + threadIdx.x / kChainDim;
    if (r >= R) return;   // (whole rows: no barrier and no cross-row operation follows)
    ChainRowModel<T, NORM, PATH, S> m{M, lcl, nl, ps, P, j, N, j < N, (int64_t)N * r + j, (int64_t)N * R};
    ChainSolveArgs ar = a;
    ar.out += 4 * r;
    onewg_tsit5<T, ChainRowModel<T, NORM, PATH, S>, false, true>(m, u0, ar, nullptr);
}

}  // namespace

// whether the trajectory solve covers this chain (no launch): the shapes of the one-workgroup solve at batch 1
bool chain_tsit5_traj_supported(const LayerConst* hlcs, int nl, int64_t P, size_t esize) {
    return chain_tsit5_shape(kChainLimits, hlcs, nl, P, 1, esize);
}

template <typename T>
hipError_t launch_kd_chain_tsit5_traj(const LayerConst* hlcs, int nl, const LayerConst* lcs, const T* p, int64_t P,
                                      const T* u0, int64_t R, const ChainSolveArgs& a, hipStream_t st) {
    if (R < 1 || R > kTrajMaxTrajectories || a.rec || a.cap != 0) return hipErrorNotSupported;
    if (!chain_tsit5_traj_supported(hlcs, nl, P, sizeof(T))) return hipErrorNotSupported;
    const size_t lds = chain_param_lds(kChainLimits, nl, P, sizeof(T));
    const unsigned grid = (unsigned)((R + kTrajPerBlock - 1) / kTrajPerBlock);
    chain_ladder(hlcs, nl, [&](auto norm, auto path, auto shape) {
        hipLaunchKernelGGL((kd_chain_tsit5_traj_kernel<T, norm(), path(), decltype(shape)>), dim3(grid),
                           dim3(kTrajBlock), lds, st, lcs, nl, p, (int)P, u0, R, a);
    });
    return hipGetLastError();
}
template hipError_t launch_kd_chain_tsit5_traj<double>(const LayerConst*, int, const LayerConst*, const double*,
                                                       int64_t, const double*, int64_t, const ChainSolveArgs&,
                                                       hipStream_t);
template hipError_t launch_kd_chain_tsit5_traj<float>(const LayerConst*, int, const LayerConst*, const float*, int64_t,
                                                      const float*, int64_t, const ChainSolveArgs&, hipStream_t);

}  // namespace kan
