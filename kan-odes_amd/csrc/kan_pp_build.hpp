// kan_pp_build.hpp — the build of kPPPerBlock intervals of one tabulated function of the pointwise KAN, as a device
// function of (block index, function, thread index within a 256-thread block).  fk_pp_build_kernel (kan_pp.hip) runs
// it once per block; the device-resident Fisher-KPP training loop (kan_small_train.hip) runs it over virtual
// blocks of one workgroup, straight into its LDS tables.  Both run this one text, so a table the loop builds has the
// bits of the launch's: the quad-of-lanes split of every evaluation and its fixed combination order, the
// Q(f - f_0) + f_0 conversion, the acceptance test and the NaN marking of a rejected interval.
#pragma once
#include "kan_common.hpp"
#include "kan_kernels.hpp"

namespace kan {

constexpr int kPPEvals = kPPCoef + kPPChecks;        // direct evaluations per interval

// What a build does about a rejected interval besides marking it: nothing, or (the diagnostic build of kan_pp.hip)
// counting it.  rejected(fn, y, f, tol·scale, interval)
struct PPBuildNoProbe {
    __device__ __forceinline__ void operator()(int, double, double, double, int) const {}
};

// LDS of a build.  The constants are shared by every block that builds from the same parameters:
//   sQ[kPPCoef²] node values -> monomial coefficients, sT[kPPEvals] nodes then check points,
//   sC[G + 1] C_0..C_{G-1}, W, sG[G] knots.
// The scratch belongs to one block: fv[kPPPerBlock][kPPEvals], sv[kPPPerBlock][kPPChecks],
// cf[kPPPerBlock][kPPCoef], then bad[kPPPerBlock] (int).
constexpr int kPPBuildFv = 0;
constexpr int kPPBuildSv = kPPBuildFv + kPPPerBlock * kPPEvals;
constexpr int kPPBuildCf = kPPBuildSv + kPPPerBlock * kPPChecks;
constexpr int kPPBuildBad = kPPBuildCf + kPPPerBlock * kPPCoef;
constexpr int kPPBuildScratch = kPPBuildBad + (kPPPerBlock * (int)sizeof(int) + 7) / 8;   // doubles
struct PPBuildLds {
    const double* sQ;
    const double* sT;
    const double* sC;
    const double* sG;
    double* scr;   // [kPPBuildScratch], this block's
};
__device__ __forceinline__ int* pp_build_bad(double* scr) { return reinterpret_cast<int*>(scr + kPPBuildBad); }

// Intervals blk·kPPPerBlock .. + kPPPerBlock of function fn into `table` ([kPPCoef/2][ni] pairs; global or LDS).
// Collective: every thread of the workgroup calls it (three block barriers); `on` is false for the threads of a
// virtual block with nothing to build (uniform over the 256 threads that share tid's block).  The caller has zeroed
// bad[] and published the constants (a barrier) before the call; bad[] holds the rejections afterwards.
template <class Probe = PPBuildNoProbe>
__device__ __forceinline__ void pp_build_block(const Math<double>& M, const LayerConst& lc, const PPConst& pc,
                                               const PPBuildLds& L, int blk, int fn, int tid, bool on,
                                               double* __restrict__ table, const Probe& rejected = Probe()) {
    const int G = lc.G;
    const double* sQ = L.sQ;
    const double* sT = L.sT;
    const double* sC = L.sC;
    const double* sG = L.sG;
    double (*fv)[kPPEvals] = reinterpret_cast<double (*)[kPPEvals]>(L.scr + kPPBuildFv);
    double (*sv)[kPPChecks] = reinterpret_cast<double (*)[kPPChecks]>(L.scr + kPPBuildSv);
    double (*cf)[kPPCoef] = reinterpret_cast<double (*)[kPPCoef]>(L.scr + kPPBuildCf);
    int* bad = pp_build_bad(L.scr);
    const int k0 = blk * kPPPerBlock;
    if (on) {
        // evaluation e = tid / 4 (all lanes of a quad take part in the shuffles)
        const int e = tid >> 2, sub = tid & 3;
        const bool live = e < kPPPerBlock * kPPEvals;
        const int kl = live ? e / kPPEvals : 0, m = live ? e - kl * kPPEvals : 0;
        const double c = pc.lo + ((double)(k0 + kl) + 0.5) * pc.w;   // exact: w is a power of two
        const double u = ::fma(sT[m], 0.5 * pc.w, c);
        const double n = normalize<NORM_RUNTIME, double>(M, lc.norm, u);
        const double invh = (double)lc.invh;
        double s = 0.0, a = 0.0, base = 0.0;    // spline-part sum, Σ|spline terms|, base term
        if (fn != PP_SWISH) {
            for (int j = sub; j < G; j += 4) {
                double aux = 0.0;
                const double y = (n - sG[j]) * invh;
                const double phi = basis_direct<double>(M, lc.basis, y, aux);
                const double t = fn == PP_PHI ? sC[j] * phi
                                              : basis_pull<double>(lc.basis, lc.iqf_quirk, y, phi, aux, sC[j]) * invh;
                s = s + t;
                a = a + kabs(t);
            }
        }
        if (sub == 3) {
            double sw, dsw;
            swish_and_grad<double>(M, u, sw, dsw);
            base = fn == PP_SWISH ? sw : (lc.use_base ? sC[G] * (fn == PP_PHI ? sw : dsw) : 0.0);
        }
        s = s + __shfl_xor(s, 1, 4);
        a = a + __shfl_xor(a, 1, 4);
        s = s + __shfl_xor(s, 2, 4);
        a = a + __shfl_xor(a, 2, 4);
        base = __shfl(base, 3, 4);
        if (live && sub == 0) {
            // acceptance scale: Σ|terms| at the point, floored at 4·w·(the function's natural
            // magnitude: Σ|C| (/h) + |W|, or 1 + |u| for swish).  The node -> monomial
            // conversion rounds at ~|Q|·eps·(variation over the interval, ~w·|f'|), so
            // where every term vanishes (swish(0) = 0) the floor keeps a correct fit from
            // being rejected; it admits absolute errors <= 2.5e-15 of that magnitude.
            // (magnitudes by compare-and-negate: with the |x| source modifier the swish branch's scale came out
            // as base + 4w(1 + u), negative below u ≈ -0.2, which rejected every swish interval there and sent
            // those points of the VJP to the direct formula; tools/pp_direct_scan.py)
            auto mag = [](double x) { return x < 0.0 ? -x : x; };
            double csum = 0.0;
            for (int j = 0; j < G; ++j) csum += mag(sC[j]);
            const double wabs = lc.use_base ? mag(sC[G]) : 0.0;
            double v, sc, ref;
            if (fn == PP_PHI) {
                v = s + base;
                sc = a + mag(base);
                ref = csum + wabs;
            } else if (fn == PP_DPHI) {
                const double dn = dnormalize<NORM_RUNTIME, double>(lc.norm, n);
                v = dn * s + base;
                sc = dn * a + mag(base);
                ref = csum * invh + wabs;
            } else {
                v = base;
                sc = mag(base);
                ref = 1.0 + mag(u);
            }
            sc += 4.0 * pc.w * ref;
            fv[kl][m] = v;
            if (m >= kPPCoef) sv[kl][m - kPPCoef] = sc;
        }
    }
    __syncthreads();
    if (on && tid < kPPPerBlock * kPPCoef) {
        // a = Q (f - f_0) + f_0 e_0: the constant is carried exactly, Q only sees the variation
        const int kl = tid / kPPCoef, i = tid - kl * kPPCoef;
        const double f0 = fv[kl][0];
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < kPPCoef; ++m) s = ::fma(sQ[i * kPPCoef + m], fv[kl][m] - f0, s);
        cf[kl][i] = i == 0 ? s + f0 : s;
    }
    __syncthreads();
    if (on && tid < kPPPerBlock * kPPChecks) {
        const int kl = tid / kPPChecks, c = tid - kl * kPPChecks;
        const double t = sT[kPPCoef + c];
        double y = cf[kl][kPPCoef - 1];
#pragma unroll
        for (int i = kPPCoef - 2; i >= 0; --i) y = ::fma(y, t, cf[kl][i]);
        if (!(kabs(y - fv[kl][kPPCoef + c]) <= pc.tol * sv[kl][c])) {
            bad[kl] = 1;
            rejected(fn, y, fv[kl][kPPCoef + c], pc.tol * sv[kl][c], k0 + kl);
        }
    }
    __syncthreads();
    if (on && tid < kPPPerBlock * kPPCoef) {
        const int kl = tid / kPPCoef, i = tid - kl * kPPCoef;
        const int64_t k = k0 + kl;
        table[((int64_t)(i >> 1) * pc.ni + k) * 2 + (i & 1)] = bad[kl] ? __builtin_nan("") : cf[kl][i];
    }
}

}  // namespace kan
