// kan_score.hip — per-edge scores of one KDense layer (gfx950): scores[o + O·i] = max_k |act(o, i, k)|, the
// quantity the reference's prune takes from activation_getter (LV_driver_KANODE.jl:79-80), without the
// [O, I, K] array kd_edge_act_kernel writes.
//
// act(o, i, k) is formed exactly as kd_edge_act_kernel forms it (the g-ascending fma chain over φ_g·C, then one
// fma with swish·W), so for the layers that kernel serves (O <= 64) the scores are the maxima of its output bit
// for bit.  The maximum keeps a NaN (nan_max): a diverged network must not look prunable.  No atomics: a block
// owns its edges over the samples it visits and writes one row of per-block maxima, rows [nkb][O·I]; with more
// than one row a second pass takes the maximum over the rows (the slab reductions' scheme).
//   kd_edge_score_k_kernel  narrow layers (O <= 64): a thread per sample k, 16 outputs of one input in registers;
//                           grid (k blocks, output tiles of 16, inputs) -- K in the 10⁵s keeps the chip busy
//   kd_edge_score_o_kernel  wide layers (O > 64): a thread per output o (coalesced C reads), the basis values of a
//                           tile of samples staged in LDS once per block; grid (output blocks, inputs, k blocks)
#include <algorithm>

#include "kan_basis.hpp"
#include "kan_common.hpp"
#include "kan_kernels.hpp"

namespace kan {

constexpr int kScoreOT = 16;    // outputs per thread of the k kernel
constexpr int kScoreKT = 128;   // samples per LDS tile of the o kernel

// max(m, a) that keeps a NaN from either side
template <typename T> __device__ __forceinline__ T nan_max(T m, T a) { return (a > m || a != a) ? a : m; }

template <typename T, int PATH>
__global__ void __launch_bounds__(kBlock)
kd_edge_score_k_kernel(const LayerConst* __restrict__ lcp, const T* __restrict__ p, const T* __restrict__ x,
                       T* __restrict__ rows, int64_t K) {
    KAN_EXP_TABLE_LDS(tab);
    __shared__ T red[kBlock / kWave][kScoreOT];
    const Math<T> M{tab};
    const LayerConst& lc = *lcp;
    const int I = lc.I, O = lc.O, G = lc.G;
    const T* __restrict__ C = p + lc.p_off;
    const T* __restrict__ W = p + lc.w_off;
    const int ob = blockIdx.y * kScoreOT;
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    T* __restrict__ row = rows + (int64_t)blockIdx.x * O * I;
    for (int i = blockIdx.z; i < I; i += gridDim.z) {
        T mx[kScoreOT];
#pragma unroll
        for (int o = 0; o < kScoreOT; ++o) mx[o] = T(0);
        for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += stride) {
            const T xi = x[(int64_t)I * k + i];
            T acc[kScoreOT];
#pragma unroll
            for (int o = 0; o < kScoreOT; ++o) acc[o] = T(0);
            BasisStream<T, PATH> bs;
            bs.init(M, lc, normalize<NORM_RUNTIME, T>(M, lc.norm, xi));
            for (int g = 0; g < G; ++g) {
                T z, aux;
                const T phi = bs.next(M, lc, g, z, aux);
                const T* Cc = C + (int64_t)O * (g + (int64_t)G * i);
#pragma unroll
                for (int o = 0; o < kScoreOT; ++o)
                    if (ob + o < O) acc[o] = kfma<T>(phi, Cc[ob + o], acc[o]);
            }
            const T sw = lc.use_base ? swish<T>(M, xi) : T(0);
#pragma unroll
            for (int o = 0; o < kScoreOT; ++o)
                if (ob + o < O) {
                    const T a = lc.use_base ? kfma<T>(sw, W[(int64_t)O * i + ob + o], acc[o]) : acc[o];
                    mx[o] = nan_max<T>(mx[o], kabs(a));
                }
        }
#pragma unroll
        for (int o = 0; o < kScoreOT; ++o) {
            T v = mx[o];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v = nan_max<T>(v, __shfl_xor(v, off, kWave));
            if (lane == 0) red[w][o] = v;
        }
        __syncthreads();
        if (threadIdx.x < kScoreOT && ob + (int)threadIdx.x < O) {
            T v = red[0][threadIdx.x];
            for (int ww = 1; ww < kBlock / kWave; ++ww) v = nan_max<T>(v, red[ww][threadIdx.x]);
            row[(int64_t)O * i + ob + threadIdx.x] = v;
        }
        __syncthreads();
    }
}

template <typename T, int PATH>
__global__ void __launch_bounds__(kBlock)
kd_edge_score_o_kernel(const LayerConst* __restrict__ lcp, const T* __restrict__ p, const T* __restrict__ x,
                       T* __restrict__ rows, int64_t K) {
    KAN_EXP_TABLE_LDS(tab);
    __shared__ T phiL[kMaxGrid * kScoreKT];   // [g][sample of the tile]
    __shared__ T swL[kScoreKT];
    const Math<T> M{tab};
    const LayerConst& lc = *lcp;
    const int I = lc.I, O = lc.O, G = lc.G;
    const T* __restrict__ C = p + lc.p_off;
    const T* __restrict__ W = p + lc.w_off;
    const int o = blockIdx.x * kBlock + threadIdx.x;
    const int64_t ntile = (K + kScoreKT - 1) / kScoreKT;
    T* __restrict__ row = rows + (int64_t)blockIdx.z * O * I;
    for (int i = blockIdx.y; i < I; i += gridDim.y) {
        const T* Ci = C + (int64_t)O * G * i;
        const T wv = (lc.use_base && o < O) ? W[(int64_t)O * i + o] : T(0);
        T mx = T(0);
        for (int64_t tile = blockIdx.z; tile < ntile; tile += gridDim.z) {
            const int64_t k0 = tile * kScoreKT;
            const int nt = (int)((K - k0) < kScoreKT ? (K - k0) : kScoreKT);
            if ((int)threadIdx.x < nt) {
                const T xi = x[(int64_t)I * (k0 + threadIdx.x) + i];
                BasisStream<T, PATH> bs;
                bs.init(M, lc, normalize<NORM_RUNTIME, T>(M, lc.norm, xi));
                for (int g = 0; g < G; ++g) {
                    T z, aux;
                    phiL[g * kScoreKT + threadIdx.x] = bs.next(M, lc, g, z, aux);
                }
                swL[threadIdx.x] = lc.use_base ? swish<T>(M, xi) : T(0);
            }
            __syncthreads();
            if (o < O) {
                for (int kk = 0; kk < nt; ++kk) {
                    T acc = T(0);
                    for (int g = 0; g < G; ++g) acc = kfma<T>(phiL[g * kScoreKT + kk], Ci[(int64_t)O * g + o], acc);
                    const T a = lc.use_base ? kfma<T>(swL[kk], wv, acc) : acc;
                    mx = nan_max<T>(mx, kabs(a));
                }
            }
            __syncthreads();
        }
        if (o < O) row[(int64_t)O * i + o] = mx;
    }
}

// scores[e] = max over the rows (ascending), NaN kept
template <typename T>
__global__ void __launch_bounds__(kBlock)
edge_score_reduce_kernel(const T* __restrict__ rows, int nrows, int64_t E, T* __restrict__ scores) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    T v = rows[e];
    for (int b = 1; b < nrows; ++b) v = nan_max<T>(v, rows[(int64_t)b * E + e]);
    scores[e] = v;
}

template <typename T, int PATH>
static hipError_t score_go(const LayerConst& hlc, const LayerConst* lc, const T* p, const T* x, T* scores, T* slab,
                           size_t slab_bytes, int64_t K, hipStream_t st) {
    const int64_t E = (int64_t)hlc.O * hlc.I;
    const int rows_cap = (int)std::min<size_t>(slab ? slab_bytes / ((size_t)E * sizeof(T)) : 0, 256);
    const int iz = std::min(hlc.I, 65535);
    int nkb;
    if (hlc.O <= 64) {
        nkb = std::max(1, std::min(grid_for(K, kBlock, 256), rows_cap));
        T* out = nkb > 1 ? slab : scores;
        const dim3 grid(nkb, (hlc.O + kScoreOT - 1) / kScoreOT, iz);
        hipLaunchKernelGGL((kd_edge_score_k_kernel<T, PATH>), grid, dim3(kBlock), 0, st, lc, p, x, out, K);
    } else {
        // a wide layer has its parallelism in the edges; the samples are split only while the grid is small
        const int ob = (hlc.O + kBlock - 1) / kBlock;
        const int64_t want = std::max<int64_t>(1, 512 / ((int64_t)ob * iz));
        nkb = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(grid_for(K, kScoreKT, 256), want), rows_cap));
        T* out = nkb > 1 ? slab : scores;
        hipLaunchKernelGGL((kd_edge_score_o_kernel<T, PATH>), dim3(ob, iz, nkb), dim3(kBlock), 0, st, lc, p, x, out,
                           K);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || nkb == 1) return e;
    hipLaunchKernelGGL((edge_score_reduce_kernel<T>), dim3((unsigned)((E + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                       slab, nkb, E, scores);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_kd_edge_scores(const LayerConst& hlc, const LayerConst* lc, const T* p, const T* x, T* scores,
                                 T* slab, size_t slab_bytes, int64_t K, hipStream_t st) {
    if (K < 1) return hipErrorInvalidValue;
    switch (hlc.path) {
    case PATH_REC_CORR: return score_go<T, PATH_REC_CORR>(hlc, lc, p, x, scores, slab, slab_bytes, K, st);
    case PATH_REC: return score_go<T, PATH_REC>(hlc, lc, p, x, scores, slab, slab_bytes, K, st);
    default: return score_go<T, PATH_DIRECT>(hlc, lc, p, x, scores, slab, slab_bytes, K, st);
    }
}

template hipError_t launch_kd_edge_scores<double>(const LayerConst&, const LayerConst*, const double*, const double*,
                                                  double*, double*, size_t, int64_t, hipStream_t);
template hipError_t launch_kd_edge_scores<float>(const LayerConst&, const LayerConst*, const float*, const float*,
                                                 float*, float*, size_t, int64_t, hipStream_t);

}  // namespace kan
