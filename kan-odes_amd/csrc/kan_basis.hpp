// kan_basis.hpp — the sequential basis generator of the column kernels (kan_col.hip, kan_score.hip).
#pragma once
#include "kan_device.hpp"

namespace kan {

// Sequential basis generator for one normalised input: direct (per-knot formula)
// or the Gaussian recurrence.
template <typename T, int PATH>
struct BasisStream {
    T n, F, R, z0, tau, invh;
    __device__ __forceinline__ void init(const Math<T>& M, const LayerConst& lc, T nn) {
        n = nn;
        invh = T(lc.invh);
        if constexpr (PATH != PATH_DIRECT) rec_anchor<T>(M, lc, n, z0, F, R, tau);   // tau = τ - τ_c
    }
    // returns φ_g, z_g (the scaled argument), aux (tanh for rswaf)
    __device__ __forceinline__ T next(const Math<T>& M, const LayerConst& lc, int g, T& z, T& aux) {
        if constexpr (PATH == PATH_DIRECT) {
            z = (n - T(lc.grid[g])) * invh;
            aux = T(0);
            return basis_direct<T>(M, lc.basis, z, aux);
        } else {
            T kc = T(lc.K[g]);
            if constexpr (PATH == PATH_REC_CORR) {
                const T e = T(lc.e[g]);
                kc = kc * kfma<T>(tau, kfma<T>(tau, T(0.5) * e * e, e), T(1));
            }
            const T v = F * kc;
            z = z0 - T(lc.Dl[g]);
            aux = T(0);
            F = F * R;
            return v;
        }
    }
};

}  // namespace kan
