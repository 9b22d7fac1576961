// kan_ens_solve.hip — R forward solves of ONE problem at R parameter vectors in one launch (gfx950): the ensemble
// twin of the one-workgroup solves kd_chain_tsit5_kernel (kan_col.hip) and fk_small_tsit5_kernel (kan_small.hip),
// for looking at what an ensemble trained (every member's trajectories over the test span, its held-out loss), for
// parameter sweeps and loss landscapes.
//
// Workgroup r = blockIdx.x is replica r: it stages p + r·P, runs onewg_tsit5 on its twin's model and writes its
// saveat rows at u_save + r·n_save·n and its counters at out + 4r.  The block index is used for nothing but these
// pointer offsets (wave-uniform, read-only before the first barrier), so replica r computes what the single launch
// computes from the same p: the kernels below restate their twins' dozen lines, the device code is shared
// (ChainModel, FkSmallModel, onewg_tsit5, pp_build_block).  No workgroup reads what another writes, there is no grid
// barrier and no spin.  u0, saveat and the options are shared by all replicas; there is no dense output (rec null,
// cap 0: no capacity stop), so a replica ends with status 0 (done) or 1 (maxiters), and one that stopped leaves the
// rows past its last reached stop as they were.
//
// The Fisher-KPP field reads φ from the PP_PHI table of ITS parameters: fk_pp_build_ens_kernel builds one table per
// replica first (grid (ni / kPPPerBlock, R); pp_build_block, the text of fk_pp_build_kernel's build, without stamps:
// an ensemble table is never reused), into a buffer that is not the handle's own table.  Two launches for any R.
#define KAN_COL_DEVICE_ONLY
#include "kan_col.hip"
#include "kan_pp_build.hpp"
#include "kan_small_fsens.hpp"

namespace kan {

namespace {

// replica r's view of the shared arguments
template <typename T>
__device__ __forceinline__ ChainSolveArgs ens_replica_args(ChainSolveArgs a, int64_t r, int64_t n) {
    if (a.u_save) a.u_save = reinterpret_cast<T*>(a.u_save) + r * a.n_save * n;
    a.out += 4 * r;
    return a;
}

// kd_chain_tsit5_kernel at p + r·P
template <typename T, int NORM, int PATH, class S>
__global__ void __launch_bounds__(kChainBlock)
kd_chain_tsit5_ens_kernel(const LayerConst* __restrict__ lcs, int nl, const T* __restrict__ p, int P,
                          const T* __restrict__ u0, int64_t B, ChainSolveArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cs_raw[];
    const int64_t r = blockIdx.x;
    LayerConst* lcl = reinterpret_cast<LayerConst*>(cs_raw);
    T* ps = reinterpret_cast<T*>(cs_raw + nl * sizeof(LayerConst));
    {
        const int nw = nl * (int)(sizeof(LayerConst) / sizeof(int32_t));
        const int32_t* src = reinterpret_cast<const int32_t*>(lcs);
        int32_t* dst = reinterpret_cast<int32_t*>(cs_raw);
        stage_chain_consts(dst, src, nw, ps, p + r * P, P);
    }
    KAN_EXP_TABLE_LDS(tab);
    __shared__ double red[kChainBlock / kWave];
    const Math<T> M{tab};
    const int N = lcl[0].I;
    const int j = threadIdx.x & (kChainDim - 1);
    const int64_t col = threadIdx.x / kChainDim;
    ChainModel<T, NORM, PATH, S> m{M, lcl, nl, ps, nullptr, P, j, 0, col < B && j < N, (int64_t)N * col + j,
                                   (int64_t)N * B};
    const ChainSolveArgs ar = ens_replica_args<T>(a, r, (int64_t)N * B);
    onewg_tsit5<T>(m, u0, ar, red);
}

// The PP_PHI table of replica blockIdx.y: fk_pp_build_kernel's build (its constants' loads, pp_build_block, the NaN
// marking of a rejected interval) at p + r·P into tables + r·stride, with no stamp read or written.  fn (PP_PHI) is
// an argument, as it is a run-time value in fk_pp_build_kernel: with the function known at compile time the
// compiler folds pp_build_block's selects away and contracts the spline sum into fmas, and the table's last bits
// are then not the launch's.
__global__ void __launch_bounds__(kBlock)
fk_pp_build_ens_kernel(const LayerConst* __restrict__ lcp, const PPConst* __restrict__ pcp,
                       const double* __restrict__ p, int P, double* __restrict__ tables, int64_t stride, int fn) {
    __shared__ double sQ[kPPCoef * kPPCoef];
    __shared__ double sT[kPPEvals];              // nodes, then check points
    __shared__ double sC[kMaxGrid + 1];          // C_0..C_{G-1}, W
    __shared__ double sG[kMaxGrid];              // knots
    __shared__ double scr[kPPBuildScratch];      // the block's scratch (kan_pp_build.hpp)
    int* bad = pp_build_bad(scr);
    const LayerConst& lc = *lcp;
    const PPConst& pc = *pcp;
    const int tid = threadIdx.x;
    const int G = lc.G;
    const int64_t r = blockIdx.y;
    const double* __restrict__ pr = p + r * P;
    if (tid < kPPCoef * kPPCoef) sQ[tid] = (&pc.Q[0][0])[tid];
    if (tid < kPPEvals) sT[tid] = tid < kPPCoef ? pc.xi[tid] : pc.tchk[tid - kPPCoef];
    if (tid <= G) sC[tid] = (tid < G || lc.use_base) ? pr[tid] : 0.0;
    if (tid < G) sG[tid] = (double)lc.grid[tid];
    if (tid < kPPPerBlock) bad[tid] = 0;
    KAN_EXP_TABLE_LDS(tab);   // its __syncthreads publishes the constants too
    const Math<double> M{tab};
    const PPBuildLds L{sQ, sT, sC, sG, scr};
    pp_build_block(M, lc, pc, L, blockIdx.x, fn, tid, true, tables + r * stride);
}

// fk_small_tsit5_kernel at p + r·P on table r (tstride: double2 between two replicas' tables)
template <int NORM, int PATH, int GT, int MAXT>
__global__ void __launch_bounds__(MAXT)
fk_small_tsit5_ens_kernel(const LayerConst* __restrict__ lcp, const double* __restrict__ p, int P,
                          const double2* __restrict__ tables, int64_t tstride, FkSmallArgs s,
                          const double* __restrict__ u0, int64_t B, ChainSolveArgs a) {
    extern __shared__ double2 tl[];
    __shared__ double red[MAXT / kWave];
    const int64_t r = blockIdx.x;
    const int fns[1] = {PP_PHI};
    stage_tables(tl, tables + r * tstride, s.ni, fns, 1);
    KAN_EXP_TABLE_LDS(tab);   // (its barrier also publishes tl)
    const Math<double> M{tab};
    const LayerConst& lc = *lcp;
    auto m = fk_small_model<NORM, PATH, GT>(M, lc, p + r * P, tl, nullptr, s, B, nullptr);
    const ChainSolveArgs ar = ens_replica_args<double>(a, r, (int64_t)s.Nx * B);
    onewg_tsit5<double>(m, u0, ar, red);
}

}  // namespace

// whether the ensemble solve covers this chain (no launch): the shapes of the one-workgroup solve
bool chain_tsit5_ens_supported(const LayerConst* hlcs, int nl, int64_t P, int64_t B, size_t esize) {
    return chain_tsit5_shape(kChainLimits, hlcs, nl, P, B, esize);
}

// the one-workgroup solve's block and dynamic LDS on a grid of n_rep workgroups
template <typename T>
hipError_t launch_kd_chain_tsit5_ens(const LayerConst* hlcs, int nl, const LayerConst* lcs, const T* p, int64_t P,
                                     const T* u0, int64_t B, const ChainSolveArgs& a, int64_t n_rep, hipStream_t st) {
    if (n_rep < 1 || n_rep > kTrainMaxReplicas || a.rec || a.cap != 0) return hipErrorNotSupported;
    if (!chain_tsit5_ens_supported(hlcs, nl, P, B, sizeof(T))) return hipErrorNotSupported;
    const size_t lds = chain_param_lds(kChainLimits, nl, P, sizeof(T));
    const int threads = chain_threads(kChainLimits, B);
    chain_ladder(hlcs, nl, [&](auto norm, auto path, auto shape) {
        hipLaunchKernelGGL((kd_chain_tsit5_ens_kernel<T, norm(), path(), decltype(shape)>), dim3((unsigned)n_rep),
                           dim3(threads), lds, st, lcs, nl, p, (int)P, u0, B, a);
    });
    return hipGetLastError();
}
template hipError_t launch_kd_chain_tsit5_ens<double>(const LayerConst*, int, const LayerConst*, const double*, int64_t,
                                                      const double*, int64_t, const ChainSolveArgs&, int64_t,
                                                      hipStream_t);
template hipError_t launch_kd_chain_tsit5_ens<float>(const LayerConst*, int, const LayerConst*, const float*, int64_t,
                                                     const float*, int64_t, const ChainSolveArgs&, int64_t, hipStream_t);

// launch_fk_small_tsit5's conditions, block and dynamic LDS; tables: [n_rep][table_stride] doubles (table_stride >=
// kPPCoef·ni, even), all of it written by the build launch before the solve launch reads it
hipError_t launch_fk_small_tsit5_ens(const LayerConst& hlc, const PPConst& hpc, const LayerConst* lc,
                                     const PPConst* pc, const double* p, int64_t P, double* tables,
                                     int64_t table_stride, const FkSmallArgs& s, const double* u0, int64_t B,
                                     const ChainSolveArgs& a, int64_t n_rep, hipStream_t st) {
    if (n_rep < 1 || n_rep > kTrainMaxReplicas || a.rec || a.cap != 0) return hipErrorNotSupported;
    if (!fk_small_supported(hlc, hpc, s.Nx, B) || s.ni != hpc.ni || hpc.ni % kPPPerBlock) return hipErrorNotSupported;
    if (!tables || table_stride < (int64_t)kPPCoef * hpc.ni || table_stride % 2 || P < hlc.G + (hlc.use_base ? 1 : 0))
        return hipErrorNotSupported;
    hipLaunchKernelGGL(fk_pp_build_ens_kernel, dim3(hpc.ni / kPPPerBlock, (unsigned)n_rep), dim3(kBlock), 0, st, lc, pc,
                       p, (int)P, tables, table_stride, (int)PP_PHI);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t lds = sizeof(double2) * (kPPCoef / 2) * (size_t)hpc.ni;
    const int threads = (int)B * kWave;
    const double2* t2 = reinterpret_cast<const double2*>(tables);
    const int64_t ts2 = table_stride / 2;
    fk_small_ladder(hlc, threads, [&](auto norm, auto path, auto gt, auto maxt) {
        hipLaunchKernelGGL((fk_small_tsit5_ens_kernel<norm(), path(), gt(), maxt()>), dim3((unsigned)n_rep),
                           dim3(threads), lds, st, lc, p, (int)P, t2, ts2, s, u0, B, a);
    });
    return hipGetLastError();
}

}  // namespace kan
