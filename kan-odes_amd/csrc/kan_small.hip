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
#include "kan_small_fsens.hpp"

namespace kan {

namespace {

// MAXT: the block bound the kernels are compiled for (256: B <= 4, one wave per SIMD and up to 256 VGPRs;
// 1024: B <= 16 at 128 VGPRs)

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
    extern __shared__ double2 tl[];
    __shared__ double red[kFsensMaxWaves];
    if constexpr (TAB) {
        const int fns[3] = {PP_PHI, PP_DPHI, PP_SWISH};
        stage_tables(tl, tables, s.ni, fns, 3);
    }
    KAN_EXP_TABLE_LDS(tab);   // (its barrier also publishes the tables)
    const Math<double> M{tab};
    constexpr int P = GT + 1;
    const int w = threadIdx.x / kWave;
    const bool sens = w > 0;   // (wave-uniform)
    const int kq = w - 1;
    const int64_t n = (int64_t)s.Nx * B;
    double* __restrict__ usave = reinterpret_cast<double*>(a.u_save);
    // a saveat stop: the values to u_save, partial k to s_save (the body of the solve: kan_small_fsens.hpp)
    auto put = [&](int64_t si, const double (&v)[E], const bool (&act)[E], const int (&e)[E]) {
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
    fk_small_fsens_body<NORM, GT, TAB, E>(M, *lcp, p, tl, red, s, u0, B, a, put);
}
}  // namespace

bool fk_small_supported(const LayerConst& hlc, const PPConst& hpc, int Nx, int64_t B) {
    return Nx >= 4 && Nx <= kWave && Nx % 2 == 0 && B >= 1 && B <= kFkSmallMaxBatch && hpc.enabled &&
           hlc.basis == BASIS_RBF && hlc.path != PATH_DIRECT && hlc.use_base &&
           (hlc.G == 10 || hlc.G == 5) && (hlc.norm == NORM_SOFTSIGN || hlc.norm == NORM_TANH_FAST);
}

hipError_t launch_fk_small_tsit5(const LayerConst& hlc, const PPConst& hpc, const LayerConst* lc, const double* p,
                                 const double* tables, const FkSmallArgs& s, const double* u0, int64_t B,
                                 const ChainSolveArgs& a, hipStream_t st) {
    if (!fk_small_supported(hlc, hpc, s.Nx, B) || s.ni != hpc.ni) return hipErrorNotSupported;
    const size_t lds = sizeof(double2) * (kPPCoef / 2) * (size_t)hpc.ni;
    const int threads = (int)B * kWave;
    fk_small_ladder(hlc, threads, [&](auto norm, auto path, auto gt, auto maxt) {
        hipLaunchKernelGGL((fk_small_tsit5_kernel<norm(), path(), gt(), maxt()>), dim3(1), dim3(threads), lds, st, lc, p,
                           (const double2*)tables, s, u0, B, a);
    });
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
    return fk_small_ladder(hlc, threads, [&](auto norm, auto path, auto gt, auto maxt) {
        const void* fn = reinterpret_cast<const void*>(&fk_small_adjoint_kernel<norm(), path(), gt(), maxt()>);
        const hipError_t e = ensure_dynamic_lds(fn, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((fk_small_adjoint_kernel<norm(), path(), gt(), maxt()>), dim3(1), dim3(threads), lds, st, lc,
                           p, (const double2*)tables, s, B, a, stage_rec);
        return hipGetLastError();
    });
}

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
    const size_t lds = sizeof(double) * fk_small_fsens_lds_doubles(tab, hpc.ni, hlc.G, two);
    if (lds > 150 * 1024) return hipErrorNotSupported;
    return fk_fsens_ladder(hlc, tab, two, [&](auto norm, auto gt, auto tb, auto e) {
        const void* fn = reinterpret_cast<const void*>(&fk_small_fsens_kernel<norm(), gt(), tb(), e()>);
        const hipError_t err = ensure_dynamic_lds(fn, lds);
        if (err != hipSuccess) return err;
        hipLaunchKernelGGL((fk_small_fsens_kernel<norm(), gt(), tb(), e()>), dim3(1), dim3(threads), lds, st, lc, p,
                           (const double2*)tables, s, u0, B, a, s_save);
        return hipGetLastError();
    });
}

}  // namespace kan
