// kan_train_loss.hpp — the loss statements of the device-resident training loops (kan_train.hip's
// kd_chain_train_lvsp_kernel, kan_train_wg.hip's kd_chain_train_wg_kernel): one wave forms the MSE, its cotangent
// and the L1 term, so both loops round them the same way.
#pragma once
#include "kan_common.hpp"

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

}  // namespace kan
