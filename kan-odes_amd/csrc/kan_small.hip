// kan_small.hip — the Fisher-KPP source-term problem at the reference's own size (PDE examples/
// Fisher-KPP_Source.jl:34-49,95-103,194-213: 26 grid points, one initial condition, T = 5, saveat 0.5,
// the default tolerances) as ONE workgroup for the whole forward solve and ONE for the whole
// InterpolatingAdjoint (the drivers of kan_onewg.hpp), instead of a host loop of per-step launches and
// host round trips over a field that fills a tenth of one wave.
//
// Layout: wave w holds trajectory w (B <= 16 waves), lane j grid point j (Nx <= 64, even: the table path's
// condition).  The periodic Laplacian's neighbours come from lanes (j ± 1) mod Nx of the same wave
// (ds_bpermute), in lap3's ascending-column order; the pointwise KAN is the piecewise-polynomial table
// (kan_pp_point.hpp) staged in LDS, with the reference formula for points off the table.  The forward is
// then the same arithmetic as the host loop's fk_rhs_pp_kernel per point, and the adjoint stage the same
// per-point pullback as the Fisher-KPP adjoint kernels (pp_vjp_point), its eleven moments block-summed per
// stage into kμ.
#include "kan_onewg.hpp"
#include "kan_lap.hpp"
#include "kan_pp_point.hpp"

namespace kan {

namespace {

// MAXT: the block bound the kernels are compiled for (256: B <= 4, one wave per SIMD and up to 256 VGPRs;
// 1024: B <= 16 at 128 VGPRs)

// The Fisher-KPP RHS and its pullback for the one-workgroup drivers.
template <int NORM, int PATH, int GT>
struct FkSmallModel {
    const Math<double>& M;
    const LayerConst& lc;
    const RecScalars<double> rc;
    const double* __restrict__ p;      // the parameters (the cold path's reference formula)
    const double2* __restrict__ tf;    // PP_PHI table (forward) or PP_DPHI (adjoint), LDS
    const double2* __restrict__ ts;    // PP_SWISH table (adjoint), LDS
    int ni;
    double inv_w, x0, cd, co;
    int Nx, j, jm, jp;                 // this lane's point and its periodic neighbours
    double* red;                       // LDS, (blockDim / 64)·(GT + 1) doubles (per-stage moment sums)
    int P;
    bool act;
    int64_t idx, n;

    __device__ double lap(double v) const {
        const double um = __shfl(v, jm, kWave), up = __shfl(v, jp, kWave);
        return lap3<double>(um, v, up, j, Nx, cd, co);
    }
    // f(y)_j = (D lap y)_j + φ(y_j)  (fk_rhs_pp_kernel: pp_pair_finish's per-point order)
    __device__ double rhs(double y) {
        const double l = lap(y);
        bool ok;
        double k = pp_eval(tf, ni, inv_w, x0, y, ok);
        if (__builtin_expect(!ok, 0)) {
            double sc;
            k = pp_direct<NORM, BASIS_RBF>(M, lc, p, lc.grid, y, sc);
        }
        return l + k;
    }
    // λsᵀ∂f/∂u at y (entry j) and kμ = Σ_points λs ∂φ/∂p, the eleven moments summed over the block
    __device__ double vjp(double y, double ls, double* __restrict__ km) {
        const double l = lap(ls);   // (D lap)ᵀ = D lap
        double S0[GT], dW;
        float S1[GT], S2[GT];
        const double xb = pp_vjp_point<NORM, PATH, GT>(M, lc, p, rc, tf, ts, ni, inv_w, x0, y, ls, S0, S1, S2, dW, true);
        double acc[GT + 1];
#pragma unroll
        for (int q = 0; q < GT; ++q) {
            const double e = lc.e[q];
            acc[q] = PATH == PATH_REC_CORR ? lc.K[q] * ::fma(lc.h2[q], (double)S2[q], ::fma(e, (double)S1[q], S0[q]))
                                           : lc.K[q] * S0[q];
        }
        acc[GT] = dW;
        block_sum_to<double, GT + 1>(acc, P, red, km);   // (ends with a block barrier)
        return act ? l + xb : 0.0;
    }
};

template <int NORM, int PATH, int GT>
__device__ __forceinline__ FkSmallModel<NORM, PATH, GT> fk_small_model(const Math<double>& M, const LayerConst& lc,
                                                                       const double* p, const double2* tf,
                                                                       const double2* ts, const FkSmallArgs& s,
                                                                       int64_t B, double* red) {
    const int j = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const bool act = j < s.Nx && w < B;
    return FkSmallModel<NORM, PATH, GT>{M, lc, RecScalars<double>(lc), p, tf, ts, s.ni, s.inv_w, s.x0, s.cd, s.co,
                                        s.Nx, j, (j + s.Nx - 1) % s.Nx, (j + 1) % s.Nx, red,
                                        GT + (lc.use_base ? 1 : 0), act, (int64_t)s.Nx * w + j,
                                        (int64_t)s.Nx * B};
}

// Stage `nt` tables of [kPPCoef/2][ni] double2 from the handle's table buffer (slots fns[0..nt)) into LDS.
__device__ __forceinline__ void stage_tables(double2* tl, const double2* __restrict__ tables, int ni, const int* fns,
                                             int nt) {
    const int tsz = (kPPCoef / 2) * ni;
    for (int f = 0; f < nt; ++f)
        for (int i = threadIdx.x; i < tsz; i += blockDim.x) tl[f * tsz + i] = tables[fns[f] * tsz + i];
}

template <int NORM, int PATH, int GT, int MAXT>
__global__ void __launch_bounds__(MAXT)
fk_small_tsit5_kernel(const LayerConst* __restrict__ lcp, const double* __restrict__ p,
                      const double2* __restrict__ tables, FkSmallArgs s, const double* __restrict__ u0, int64_t B,
                      ChainSolveArgs a) {
    extern __shared__ double2 tl[];
    __shared__ double red[MAXT / kWave];
    const int fns[1] = {PP_PHI};
    stage_tables(tl, tables, s.ni, fns, 1);
    KAN_EXP_TABLE_LDS(tab);   // (its barrier also publishes tl)
    const Math<double> M{tab};
    const LayerConst& lc = *lcp;
    auto m = fk_small_model<NORM, PATH, GT>(M, lc, p, tl, nullptr, s, B, nullptr);
    onewg_tsit5<double>(m, u0, a, red);
}

template <int NORM, int PATH, int GT, int MAXT>
__global__ void __launch_bounds__(MAXT)
fk_small_adjoint_kernel(const LayerConst* __restrict__ lcp, const double* __restrict__ p,
                        const double2* __restrict__ tables, FkSmallArgs s, int64_t B, ChainAdjointArgs a,
                        int stage_rec) {
    extern __shared__ double2 tl[];
    __shared__ double red[MAXT / kWave];
    __shared__ double mred[(MAXT / kWave) * (GT + 1)];
    const int tsz = (kPPCoef / 2) * s.ni;
    const int fns[2] = {PP_DPHI, PP_SWISH};
    stage_tables(tl, tables, s.ni, fns, 2);
    const int P = GT + 1;   // (the launcher admits use_base layers only)
    double* mu = reinterpret_cast<double*>(tl + 2 * tsz);   // [2][P]
    double* km = mu + 2 * P;                                // [7][P]
    double* tsl = km + 7 * P;                               // [nsteps]
    double* dtsl = tsl + a.nsteps;
    for (int i = threadIdx.x; i < 9 * P; i += blockDim.x) mu[i] = 0.0;
    for (int64_t i = threadIdx.x; i < a.nsteps; i += blockDim.x) {
        tsl[i] = a.ts[i];
        dtsl[i] = a.dts[i];
    }
    KAN_EXP_TABLE_LDS(tab);
    const Math<double> M{tab};
    const LayerConst& lc = *lcp;
    double* recl = nullptr;
    if (stage_rec) {
        recl = dtsl + a.nsteps;
        onewg_stage_rec<double>(recl, a, (int64_t)s.Nx * B);
    }
    auto m = fk_small_model<NORM, PATH, GT>(M, lc, p, tl, tl + tsz, s, B, mred);
    onewg_adjoint<double>(m, a, mu, km, tsl, dtsl, red, recl);
}


// ---- forward sensitivities (SciMLSensitivity 7.69 ForwardDiffSensitivity) ---------------------------------
// The reference's Fisher-KPP gradient at its own size: Zygote.gradient(x -> loss(x), p) with no sensealg
// (Fisher-KPP_Source.jl:198; the Allen-Cahn source driver likewise).  With length(u0) + length(p) = 26 + 11
// <= 100 SciMLSensitivity picks ForwardDiffSensitivity: the solve runs over ForwardDiff.Dual numbers with one
// partial per parameter (chunk = P = 11), i.e. over the state [u; S_1..S_P], S_k = ∂u/∂p_k, with
//     S_k' = (D lap) S_k + φ'(u) S_k + ∂φ/∂p_k(u),   ∂φ/∂C_k = B_k(N(u)),  ∂φ/∂W = swish(u)
// (kdense.jl:116-124), integrated by the same Tsit5 (third-party semantics, restated from the pinned
// SciMLSensitivity 7.69 / DiffEqBase / OrdinaryDiffEq 6.89; verify where Julia exists).  What the Dual solve
// changes in the step control: DiffEqBase's ODE_DEFAULT_NORM over Dual numbers counts the partials.  The
// residual scale of state entry i is abstol + reltol·max(‖u_i‖, ‖unew_i‖) with ‖x‖ = sqrt(value² + Σ_k
// partial_k²) (calculate_residuals calls the scalar Dual norm), the residual's value and partials are divided by
// it, and EEst = sqrt(Σ_i (value² + Σ_k partial_k²) / (n·(1 + P))); the Hairer-Wanner initial step takes the same
// norms; saveat values and partials come from the same interpolant.
//
// Layout: wave 0 carries the values, wave 1 + k the partial S_k (k < G: C_k, k = G: W); lane l is point l % Nx
// of trajectory l / Nx (Nx·B <= 64).  Wave 0 alone evaluates the RHS at the values and hands φ'(y), swish(y) and
// N(y) of every stage to the partial waves through LDS (one barrier per stage, two slots); a partial wave's
// evaluation is then a stencil, an fma and one exponential.  The other exchanges are the per-entry Dual norms (one
// LDS round per step) and the error norm's block sum.  TAB: φ, φ' and swish from the
// piecewise-polynomial tables (PP_PHI, PP_DPHI, PP_SWISH staged in LDS, the reference formula off the table);
// otherwise the reference formula throughout (odd Nx, table path off).
//
// E: state entries per lane.  E = 1 is the layout above.  E = 2 (64 < Nx·B <= 128): lane l carries entries l and
// l + 64, every per-entry statement is the one above written once per entry, and the LDS rows (the exchange and the
// two slots) are 128 columns.  A stencil neighbour e' lives in lane e' & 63, half e' >> 6: a trajectory may straddle
// entry 64, and its periodic wrap may cross the halves.  A lane gives lo + hi to the block sums, so with an empty
// upper half (Nx·B <= 64) every sum has the bits of E = 1.
template <int NORM, int GT, bool TAB, int E>
__global__ void __launch_bounds__((GT + 2) * kWave)
fk_small_fsens_kernel(const LayerConst* __restrict__ lcp, const double* __restrict__ p,
                      const double2* __restrict__ tables, FkSmallArgs s, const double* __restrict__ u0, int64_t B,
                      ChainSolveArgs a, double* __restrict__ s_save) {
    using K = Tsit5Tab;
    extern __shared__ double2 tl[];
    __shared__ double red[kFsensMaxWaves];
    const int tsz = TAB ? (kPPCoef / 2) * s.ni : 0;
    if constexpr (TAB) {
        const int fns[3] = {PP_PHI, PP_DPHI, PP_SWISH};
        stage_tables(tl, tables, s.ni, fns, 3);
    }
    constexpr int W = E * kWave;                                         // entries per LDS row
    double* __restrict__ xv = reinterpret_cast<double*>(tl + 3 * tsz);   // [waves][W] per-entry exchange
    KAN_EXP_TABLE_LDS(tab);   // (its barrier also publishes the tables)
    const Math<double> M{tab};
    const LayerConst& lc = *lcp;
    constexpr int P = GT + 1;
    const int w = threadIdx.x / kWave, l = threadIdx.x & (kWave - 1);
    const int nw = (int)(blockDim.x / kWave);
    const int Nx = s.Nx;
    const int64_t n = (int64_t)Nx * B;
    // entry h of this lane: e[h] = l + 64 h, point j[h] of its trajectory, neighbours jm[h] / jp[h] (entry indices;
    // an inactive entry points at itself)
    bool act[E];
    int e[E], j[E], jm[E], jp[E];
#pragma unroll
    for (int h = 0; h < E; ++h) {
        e[h] = l + h * kWave;
        act[h] = e[h] < n;
        j[h] = e[h] % Nx;
        const int b0 = e[h] - j[h];
        jm[h] = act[h] ? b0 + (j[h] + Nx - 1) % Nx : e[h];
        jp[h] = act[h] ? b0 + (j[h] + 1) % Nx : e[h];
    }
    const bool sens = w > 0;   // (wave-uniform)
    const int kq = w - 1;
    const double2* tphi = tl;
    const double2* tdphi = tl + tsz;
    const double2* tsw = tl + 2 * tsz;
    // v at entry q of this wave (lane q & 63, half q >> 6)
    auto at = [&](const double (&v)[E], int q) -> double {
        if constexpr (E == 1) {
            return __shfl(v[0], q, kWave);
        } else {
            const double lo = __shfl(v[0], q & (kWave - 1), kWave), hi = __shfl(v[1], q & (kWave - 1), kWave);
            return q >= kWave ? hi : lo;
        }
    };
    // E = 2: the four neighbour entries (7 bits each) and the first / last-point flags of both entries in one
    // register, unpacked where they are used (what is derived from them is loop-invariant, and kept unpacked
    // across the step loop it costs the registers this kernel does not have)
    unsigned nbr = 0;
    if constexpr (E > 1) {
#pragma unroll
        for (int h = 0; h < E; ++h)
            nbr |= (unsigned)(jm[h] | (jp[h] << 7)) << (14 * h) | (unsigned)(j[h] == 0) << (28 + 2 * h) |
                   (unsigned)(j[h] == Nx - 1) << (29 + 2 * h);
    }
    auto lap = [&](const double (&v)[E], int h) -> double {
        if constexpr (E == 1) {
            const double um = at(v, jm[h]), up = at(v, jp[h]);
            return lap3<double>(um, v[h], up, j[h], Nx, s.cd, s.co);
        } else {
            unsigned pk = nbr;
            asm volatile("" : "+v"(pk));   // (opaque here: nothing unpacked is hoisted out of the step loop)
            const double um = at(v, (int)(pk >> (14 * h)) & 127), up = at(v, (int)(pk >> (14 * h + 7)) & 127);
            const int i = (pk >> (28 + 2 * h)) & 1 ? 0 : ((pk >> (29 + 2 * h)) & 1 ? Nx - 1 : 1);   // (Nx >= 3)
            return lap3<double>(um, v[h], up, i, Nx, s.cd, s.co);
        }
    };
    // One evaluation of the Dual RHS at the stage input z (wave 0: the values y; wave 1 + k: the partial s_k):
    //   wave 0:      f(y) = (D lap y) + φ(y)                    (FkSmallModel::rhs), and the quantities every
    //                partial needs at y -- φ'(y), swish(y), N(y) -- into LDS slot `slot`;
    //   wave 1 + k:  ((D lap) s_k + s_k φ'(y)) + ∂φ/∂p_k(y),  ∂φ/∂C_k = B_k(N(y)) by the reference formula,
    //                ∂φ/∂W = swish(y), read from that slot after the block barrier.
    // Only wave 0 evaluates at the values, so a partial wave costs a stencil, one fma and one exponential.
    // [2][3][W]: φ', swish, N by slot (E = 2: after the exchange rows of this block's G + 2 waves)
    double* __restrict__ shv = xv + (E == 1 ? kFsensMaxWaves : GT + 2) * W;
    auto F = [&](const double (&z)[E], int slot, double (&r)[E]) {
        double* sh = shv + slot * 3 * W;
        if (!sens) {
#pragma unroll
            for (int h = 0; h < E; ++h) {
                const double lp = lap(z, h);
                double k = 0.0, dphi = 0.0, sw = 0.0;
                bool ok = false, ok2 = false;
                if constexpr (TAB) {
                    k = pp_eval(tphi, s.ni, s.inv_w, s.x0, z[h], ok);
                    ok2 = pp_eval2<true>(tdphi, tsw, s.ni, s.inv_w, s.x0, z[h], dphi, sw);
                }
                if (!ok) {
                    double sc;
                    k = pp_direct<NORM, BASIS_RBF>(M, lc, p, lc.grid, z[h], sc);
                }
                if (!ok2) pp_direct_dphi_sw<NORM, BASIS_RBF>(M, lc, p, z[h], dphi, sw);
                r[h] = lp + k;
                sh[e[h]] = dphi;
                sh[W + e[h]] = sw;
                sh[2 * W + e[h]] = normalize<NORM, double>(M, lc.norm, z[h]);
                if constexpr (E > 1) __builtin_amdgcn_sched_barrier(0);   // (one entry's evaluation at a time: registers)
            }
        }
        __syncthreads();
        if (sens) {
#pragma unroll
            for (int h = 0; h < E; ++h) {
                const double lp = lap(z, h);
                const double dphi = sh[e[h]];
                double dp = sh[W + e[h]];
                if (kq < GT) {
                    const double y = (sh[2 * W + e[h]] - (double)lc.grid[kq]) * (double)lc.invh;
                    double aux;
                    dp = basis_direct<double>(M, BASIS_RBF, y, aux);
                }
                r[h] = (lp + z[h] * dphi) + dp;
                if constexpr (E > 1) __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    // Σ over the waves of v at each of this lane's entries (value first, then the partials in order: the entry's
    // Dual sse), the same totals in every wave; v of an inactive entry counts as zero
    auto pt_sum = [&](const double (&v)[E], double (&t)[E]) {
#pragma unroll
        for (int h = 0; h < E; ++h) xv[w * W + e[h]] = act[h] ? v[h] : 0.0;
        __syncthreads();
#pragma unroll
        for (int h = 0; h < E; ++h) {
            t[h] = xv[e[h]];
            for (int q = 1; q < nw; ++q) t[h] += xv[q * W + e[h]];
        }
        __syncthreads();
    };
    // Σ over the block of v at the active entries (a lane gives lo + hi)
    auto bsum = [&](const double (&v)[E]) -> double {
        double t = act[0] ? v[0] : 0.0;
#pragma unroll
        for (int h = 1; h < E; ++h) t += act[h] ? v[h] : 0.0;
        return onewg_bsum(t, red);
    };
    double* __restrict__ usave = reinterpret_cast<double*>(a.u_save);
    auto put = [&](int64_t si, const double (&v)[E]) {
#pragma unroll
        for (int h = 0; h < E; ++h) {
            if (!act[h]) continue;
            if (!sens) {
                if (usave) usave[si * n + e[h]] = v[h];
            } else if (s_save) {
                s_save[(si * P + kq) * n + e[h]] = v[h];
            }
        }
    };
    // this wave's entries of the Dual state (the value, or partial kq) and their seven stage values.  E = 2: the
    // upper entry's stage values (rows 0-6), and inside the step loop both entries' state and norm (rows 7-10), are
    // parked in LDS ([waves][11][64], this lane's own column: no other thread reads it), so that what is carried
    // across an evaluation fits the 168 registers of G + 2 = 12 waves
    double z[E], kr[7], sq[E], fr[E];
    double* kl = shv + 2 * 3 * W + w * 11 * kWave + l;
    auto k = [&](int q, int h) -> double {
        if constexpr (E == 1) return kr[q];
        else return h == 0 ? kr[q] : kl[q * kWave];
    };
    auto kset = [&](int q, const double (&r)[E]) {
        kr[q] = r[0];
        if constexpr (E > 1) kl[q * kWave] = r[1];
    };
#pragma unroll
    for (int h = 0; h < E; ++h) z[h] = sens ? 0.0 : (act[h] ? u0[e[h]] : 0.0);
    // (slot 1: stage 0 of the first step follows on slot 0; when the step is fixed no barrier lies in between)
    F(z, 1, fr);
    kset(0, fr);
    const double t0 = a.t0, tf = a.tf;
    const double ntot = (double)n * (double)(P + 1);
    int64_t si = 0;
    while (si < a.n_save && a.saveat[si] <= t0 + 1e-14 * ::fmax(1.0, ::fabs(t0))) {
        put(si, z);
        ++si;
    }
    double nrm[E];   // ‖u_i‖ of each of this lane's entries (the Dual norm over value and partials)
#pragma unroll
    for (int h = 0; h < E; ++h) nrm[h] = 0.0;
    if (a.adaptive) {
#pragma unroll
        for (int h = 0; h < E; ++h) sq[h] = z[h] * z[h];
        pt_sum(sq, nrm);
#pragma unroll
        for (int h = 0; h < E; ++h) nrm[h] = ::sqrt(nrm[h]);
    }
    double dt = a.dt;
    if (a.adaptive && !(a.dt > 0)) {   // Hairer & Wanner over the Dual state
        double sk[E], y1[E], f1[E];
#pragma unroll
        for (int h = 0; h < E; ++h) {
            sk[h] = ::fma(a.reltol, nrm[h], a.abstol);
            const double e0 = z[h] / sk[h];
            sq[h] = e0 * e0;
        }
        const double d0 = ::sqrt(bsum(sq) / ntot);
#pragma unroll
        for (int h = 0; h < E; ++h) {
            const double e1 = k(0, h) / sk[h];
            sq[h] = e1 * e1;
        }
        const double d1 = ::sqrt(bsum(sq) / ntot);
        double dt0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
        dt0 = ::fmin(dt0, tf - t0);
#pragma unroll
        for (int h = 0; h < E; ++h) y1[h] = ::fma(dt0, k(0, h), z[h]);
        F(y1, 1, f1);
#pragma unroll
        for (int h = 0; h < E; ++h) {
            const double er = ::fma(-1.0, k(0, h), f1[h]) / sk[h];
            sq[h] = er * er;
        }
        const double d2 = ::sqrt(bsum(sq) / ntot) / dt0;
        const double mx = ::fmax(d1, d2);
        const double dt1 = mx <= 1e-15 ? ::fmax(1e-6, dt0 * 1e-3) : ::pow(0.01 / mx, 1.0 / 5.0);
        dt = ::fmin(::fmin(100 * dt0, dt1), tf - t0);
    }
    auto zv = [&](int h) -> double {   // (the step loop's reads of the state and its norm)
        if constexpr (E == 1) return z[0];
        else return kl[(h == 0 ? 9 : 7) * kWave];
    };
    auto nv = [&](int h) -> double {
        if constexpr (E == 1) return nrm[0];
        else return kl[(h == 0 ? 10 : 8) * kWave];
    };
    if constexpr (E > 1) {
        kl[7 * kWave] = z[1];
        kl[8 * kWave] = nrm[1];
        kl[9 * kWave] = z[0];
        kl[10 * kWave] = nrm[0];
    }
    double qold = a.qoldinit, t = t0;
    int64_t naccept = 0, nreject = 0, nf = 0, it = 0, status = 0;
    for (; it < a.maxiters; ++it) {
        if (t >= tf - 1e-14 * ::fmax(1.0, ::fabs(tf))) break;
        dt = ::fmin(dt, tf - t);
        double y[E];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int h = 0; h < E; ++h) {
                y[h] = zv(h);
#pragma unroll
                for (int q = 0; q <= i; ++q) y[h] = ::fma(dt * K::TA[i][q], k(q, h), y[h]);
            }
            F(y, i & 1, fr);
            kset(i + 1, fr);
        }
        nf += 6;
        double dtnew = dt, nn[E];
#pragma unroll
        for (int h = 0; h < E; ++h) nn[h] = nv(h);
        if (a.adaptive) {
            double er[E];
#pragma unroll
            for (int h = 0; h < E; ++h) {
                double ev = 0.0;
#pragma unroll
                for (int q = 0; q < 6; ++q) ev = ::fma(dt * K::BT[q], k(q, h), ev);
                er[h] = ::fma(dt * K::BT[6], k(6, h), ev);
                sq[h] = y[h] * y[h];
            }
            pt_sum(sq, nn);
#pragma unroll
            for (int h = 0; h < E; ++h) {
                nn[h] = ::sqrt(nn[h]);
                const double sk = ::fma(a.reltol, ::fmax(nv(h), nn[h]), a.abstol);
                const double r = er[h] / sk;
                sq[h] = r * r;
            }
            const double eest = ::sqrt(bsum(sq) / ntot);
            const double q11 = eest > 0 ? ::pow(eest, a.beta1) : 0.0;
            if (eest > 1.0 && dt > a.dtmin) {
                ++nreject;
                dt = dt / ::fmin(1.0 / a.qmin, q11 / a.gamma);
                continue;
            }
            double q = q11 / ::pow(qold, a.beta2);
            q = ::fmax(1.0 / a.qmax, ::fmin(1.0 / a.qmin, q / a.gamma));
            if (1.0 <= q && q <= 1.0) q = 1.0;   // qsteady_min = qsteady_max = 1
            dtnew = q > 0 ? dt / q : dt * a.qmax;
            qold = ::fmax(eest, a.qoldinit);
        }
        const double tn = t + dt;
        while (si < a.n_save && a.saveat[si] <= tn + 1e-12 * ::fmax(1.0, ::fabs(tn))) {
            const double tsv = a.saveat[si];
            double v[E];
#pragma unroll
            for (int h = 0; h < E; ++h) v[h] = y[h];
            if (!(::fabs(tsv - tn) <= 1e-12 * ::fmax(1.0, ::fabs(tn)))) {
                double wt[7];
                tsit5_interp_weights((tsv - t) / dt, wt);
#pragma unroll
                for (int h = 0; h < E; ++h) {
                    v[h] = zv(h);
#pragma unroll
                    for (int q = 0; q < 7; ++q) v[h] = ::fma(wt[q] * dt, k(q, h), v[h]);
                }
            }
            put(si, v);
            ++si;
        }
        if (a.ts && threadIdx.x == 0 && naccept < a.cap) {   // the accepted steps (diagnostics: step-size replay)
            a.ts[naccept] = t;
            a.dts[naccept] = dt;
        }
        kr[0] = kr[6];   // commit (value and partials), FSAL
        if constexpr (E == 1) {
            z[0] = y[0];
            nrm[0] = nn[0];
        } else {
            kl[0] = kl[6 * kWave];
            kl[7 * kWave] = y[1];
            kl[8 * kWave] = nn[1];
            kl[9 * kWave] = y[0];
            kl[10 * kWave] = nn[0];
        }
        t = tn;
        ++naccept;
        dt = dtnew;
    }
    if (it == a.maxiters && !(t >= tf - 1e-14 * ::fmax(1.0, ::fabs(tf)))) status = 1;
    if (threadIdx.x == 0) {
        a.out[0] = naccept;
        a.out[1] = nreject;
        a.out[2] = nf + 1;
        a.out[3] = status;
    }
}
}  // namespace

bool fk_small_supported(const LayerConst& hlc, const PPConst& hpc, int Nx, int64_t B) {
    return Nx >= 4 && Nx <= kWave && Nx % 2 == 0 && B >= 1 && B <= kFkSmallMaxBatch && hpc.enabled &&
           hlc.basis == BASIS_RBF && hlc.path != PATH_DIRECT && hlc.use_base &&
           (hlc.G == 10 || hlc.G == 5) && (hlc.norm == NORM_SOFTSIGN || hlc.norm == NORM_TANH_FAST);
}

#define KAN_SMALL_GO(KERNEL, ...)                                                                                   \
    do {                                                                                                          \
        if (hlc.path == PATH_REC_CORR) {                                                                          \
            if (hlc.G == 10 && hlc.norm == NORM_SOFTSIGN) KERNEL(NORM_SOFTSIGN, PATH_REC_CORR, 10);               \
            else if (hlc.G == 10) KERNEL(NORM_TANH_FAST, PATH_REC_CORR, 10);                                      \
            else if (hlc.norm == NORM_SOFTSIGN) KERNEL(NORM_SOFTSIGN, PATH_REC_CORR, 5);                          \
            else KERNEL(NORM_TANH_FAST, PATH_REC_CORR, 5);                                                        \
        } else {                                                                                                  \
            if (hlc.G == 10 && hlc.norm == NORM_SOFTSIGN) KERNEL(NORM_SOFTSIGN, PATH_REC, 10);                    \
            else if (hlc.G == 10) KERNEL(NORM_TANH_FAST, PATH_REC, 10);                                           \
            else if (hlc.norm == NORM_SOFTSIGN) KERNEL(NORM_SOFTSIGN, PATH_REC, 5);                               \
            else KERNEL(NORM_TANH_FAST, PATH_REC, 5);                                                             \
        }                                                                                                         \
    } while (0)

hipError_t launch_fk_small_tsit5(const LayerConst& hlc, const PPConst& hpc, const LayerConst* lc, const double* p,
                                 const double* tables, const FkSmallArgs& s, const double* u0, int64_t B,
                                 const ChainSolveArgs& a, hipStream_t st) {
    if (!fk_small_supported(hlc, hpc, s.Nx, B) || s.ni != hpc.ni) return hipErrorNotSupported;
    const size_t lds = sizeof(double2) * (kPPCoef / 2) * (size_t)hpc.ni;
    const int threads = (int)B * kWave;
#define KAN_SMALL_FWD(NORM, PATH, GT)                                                                              \
    do {                                                                                                         \
        if (threads <= 256)                                                                                      \
            hipLaunchKernelGGL((fk_small_tsit5_kernel<NORM, PATH, GT, 256>), dim3(1), dim3(threads), lds, st, lc, p, \
                               (const double2*)tables, s, u0, B, a);                                             \
        else                                                                                                     \
            hipLaunchKernelGGL((fk_small_tsit5_kernel<NORM, PATH, GT, 1024>), dim3(1), dim3(threads), lds, st, lc, \
                               p, (const double2*)tables, s, u0, B, a);                                          \
    } while (0)
    KAN_SMALL_GO(KAN_SMALL_FWD);
#undef KAN_SMALL_FWD
    return hipGetLastError();
}

hipError_t launch_fk_small_adjoint(const LayerConst& hlc, const PPConst& hpc, const LayerConst* lc, const double* p,
                                   const double* tables, const FkSmallArgs& s, int64_t B, const ChainAdjointArgs& a,
                                   hipStream_t st) {
    if (!fk_small_supported(hlc, hpc, s.Nx, B) || s.ni != hpc.ni || a.nsteps < 1) return hipErrorNotSupported;
    const int P = hlc.G + 1;
    size_t lds = 2 * sizeof(double2) * (kPPCoef / 2) * (size_t)hpc.ni + sizeof(double) * (9 * (size_t)P + 2 * a.nsteps);
    if (lds > 150 * 1024) return hipErrorNotSupported;   // (~6,000 forward steps at ni = 256)
    // the forward's dense output staged in LDS too where it fits (the reference's 26-point problem: ~45 steps,
    // 65 KB): every adjoint stage interpolates it
    const size_t rec = sizeof(double) * ((size_t)a.nsteps * 7 + 1) * (size_t)s.Nx * B;
    const int stage_rec = lds + rec <= 150 * 1024 ? 1 : 0;
    if (stage_rec) lds += rec;
    const int threads = (int)B * kWave;
#define KAN_SMALL_ADJ1(NORM, PATH, GT, MAXT)                                                                       \
    do {                                                                                                         \
        {                                                                                                        \
            const void* fn = reinterpret_cast<const void*>(&fk_small_adjoint_kernel<NORM, PATH, GT, MAXT>);        \
            hipError_t e_ = ensure_dynamic_lds(fn, lds);                                                         \
            if (e_ != hipSuccess) return e_;                                                                     \
        }                                                                                                        \
        hipLaunchKernelGGL((fk_small_adjoint_kernel<NORM, PATH, GT, MAXT>), dim3(1), dim3(threads), lds, st, lc, p, \
                           (const double2*)tables, s, B, a, stage_rec);                                          \
    } while (0)
#define KAN_SMALL_ADJ(NORM, PATH, GT)                                                                              \
    do {                                                                                                         \
        if (threads <= 256) KAN_SMALL_ADJ1(NORM, PATH, GT, 256);                                                 \
        else KAN_SMALL_ADJ1(NORM, PATH, GT, 1024);                                                               \
    } while (0)
    KAN_SMALL_GO(KAN_SMALL_ADJ);
#undef KAN_SMALL_ADJ
#undef KAN_SMALL_ADJ1
    return hipGetLastError();
}
#undef KAN_SMALL_GO

// wide (KANODE_OPT_FSENS_WIDE): 0 = the one-entry kernel alone (Nx·B <= 64); 1 = the two-entry kernel above 64
// entries, up to 128; 2 = the two-entry kernel for every Nx·B <= 128 (tests)
bool fk_small_fsens_supported(const LayerConst& hlc, int Nx, int64_t B, int wide) {
    const int P = hlc.G + 1;
    return Nx >= 3 && B >= 1 && (int64_t)Nx * B <= (wide ? 2 : 1) * kWave && P + 1 <= kFsensMaxWaves &&
           hlc.basis == BASIS_RBF && hlc.use_base && (hlc.G == 10 || hlc.G == 5) &&
           (hlc.norm == NORM_SOFTSIGN || hlc.norm == NORM_TANH_FAST);
}

hipError_t launch_fk_small_fsens(const LayerConst& hlc, const PPConst& hpc, bool tab, const LayerConst* lc,
                                 const double* p, const double* tables, const FkSmallArgs& s, const double* u0,
                                 int64_t B, const ChainSolveArgs& a, double* s_save, int wide, hipStream_t st) {
    if (!fk_small_fsens_supported(hlc, s.Nx, B, wide) || (tab && (!hpc.enabled || s.ni != hpc.ni || !tables)))
        return hipErrorNotSupported;
    const int threads = (hlc.G + 2) * kWave;
    const bool two = wide == 2 || (int64_t)s.Nx * B > kWave;   // entries per lane
    const size_t lds = (tab ? 3 * sizeof(double2) * (kPPCoef / 2) * (size_t)hpc.ni : 0) +
                       (two ? sizeof(double) * ((size_t)(hlc.G + 2 + 6) * 2 * kWave +   // exchange + the two slots
                                                11 * (size_t)threads)                  // + the parked state
                            : sizeof(double) * (size_t)(kFsensMaxWaves + 6) * kWave);
    if (lds > 150 * 1024) return hipErrorNotSupported;
#define KAN_FSENS2(NORM, GT, TAB, E)                                                                               \
    do {                                                                                                         \
        const void* fn = reinterpret_cast<const void*>(&fk_small_fsens_kernel<NORM, GT, TAB, E>);                \
        hipError_t e_ = ensure_dynamic_lds(fn, lds);                                                             \
        if (e_ != hipSuccess) return e_;                                                                         \
        hipLaunchKernelGGL((fk_small_fsens_kernel<NORM, GT, TAB, E>), dim3(1), dim3(threads), lds, st, lc, p,      \
                           (const double2*)tables, s, u0, B, a, s_save);                                         \
    } while (0)
#define KAN_FSENS1(NORM, GT, TAB)                                                                                  \
    do {                                                                                                         \
        if (two) KAN_FSENS2(NORM, GT, TAB, 2);                                                                   \
        else KAN_FSENS2(NORM, GT, TAB, 1);                                                                       \
    } while (0)
#define KAN_FSENS(NORM, GT)                                                                                        \
    do {                                                                                                         \
        if (tab) KAN_FSENS1(NORM, GT, true);                                                                     \
        else KAN_FSENS1(NORM, GT, false);                                                                        \
    } while (0)
    if (hlc.G == 10 && hlc.norm == NORM_SOFTSIGN) KAN_FSENS(NORM_SOFTSIGN, 10);
    else if (hlc.G == 10) KAN_FSENS(NORM_TANH_FAST, 10);
    else if (hlc.norm == NORM_SOFTSIGN) KAN_FSENS(NORM_SOFTSIGN, 5);
    else KAN_FSENS(NORM_TANH_FAST, 5);
#undef KAN_FSENS
#undef KAN_FSENS1
#undef KAN_FSENS2
    return hipGetLastError();
}

}  // namespace kan
