// kan_small_fsens.hpp — the device code the one-workgroup Fisher-KPP kernels share: the RHS model of the plain
// solve / adjoint (FkSmallModel, for the drivers of kan_onewg.hpp) and the body of the forward-sensitivity (Dual)
// solve, parameterised on what happens at a saveat stop.  fk_small_fsens_kernel (kan_small.hip) stores the stop's
// values and partials; the device-resident training loop (kan_small_train.hip) accumulates the loss and the
// gradient from them instead.
#pragma once
#include "kan_onewg.hpp"
#include "kan_lap.hpp"
#include "kan_pp_point.hpp"

namespace kan {

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
                                                                       int64_t B, double* red,
                                                                       int tid = (int)threadIdx.x) {
    const int j = tid & (kWave - 1), w = tid / kWave;
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

// The dynamic LDS of the Dual solve below, in doubles: the three tables (TAB), the exchange rows, the two slots and,
// at two entries per lane, the parked state (launch_fk_small_fsens's budget; the training loop's rows follow it).
__host__ __device__ inline size_t fk_small_fsens_lds_doubles(bool tab, int ni, int G, bool two) {
    return (tab ? 3 * (size_t)kPPCoef * (size_t)ni : 0) +
           (two ? (size_t)(G + 2 + 6) * 2 * kWave +         // exchange + the two slots
                      11 * (size_t)(G + 2) * kWave          // + the parked state
                : (size_t)(kFsensMaxWaves + 6) * kWave);
}

// The forward-sensitivity solve of kan_small.hip's header comment (layout, E, TAB as described there), as the
// body of a kernel of G + 2 waves: every thread of the block calls it.  tl: the dynamic LDS (the PP_PHI, PP_DPHI,
// PP_SWISH tables when TAB, then this solve's rows); red: kFsensMaxWaves doubles of LDS; p: the parameters of the
// reference formula (global, or an LDS copy where the kernel itself changes them).  a's pointers may be LDS
// addresses; a.u_save is not used here.  tid: threadIdx.x (a kernel that loops over solves passes it opaque, so that
// nothing derived from the lane is hoisted out of its loop; the block sums of kan_onewg.hpp read threadIdx.x
// themselves).  At saveat stop si every thread calls put(si, v, act, e) with its entries'
// values (wave 0) or partials (wave 1 + k) at the stop: block-uniform control flow, so put may hold barriers.
template <int NORM, int GT, bool TAB, int E, class Put>
__device__ __forceinline__ void fk_small_fsens_body(const Math<double>& M, const LayerConst& lc, const double* p,
                                                    double2* tl, double* red, const FkSmallArgs& s,
                                                    const double* __restrict__ u0, int64_t B,
                                                    const ChainSolveArgs& a, Put& put,
                                                    int tid = (int)threadIdx.x) {
    using K = Tsit5Tab;
    const int tsz = TAB ? (kPPCoef / 2) * s.ni : 0;
    constexpr int W = E * kWave;                                         // entries per LDS row
    double* __restrict__ xv = reinterpret_cast<double*>(tl + 3 * tsz);   // [waves][W] per-entry exchange
    constexpr int P = GT + 1;
    const int w = tid / kWave, l = tid & (kWave - 1);
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
        put(si, z, act, e);
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
            put(si, v, act, e);
            ++si;
        }
        if (a.ts && tid == 0 && naccept < a.cap) {   // the accepted steps (diagnostics: step-size replay)
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
    if (tid == 0) {
        a.out[0] = naccept;
        a.out[1] = nreject;
        a.out[2] = nf + 1;
        a.out[3] = status;
    }
}

// ---- the specialisation ladders of the small-field launchers (host) ----------------------------------------------
// The plain solve and the adjoint of a field fk_small_supported accepts: go(norm, path, gt, maxt) with PATH_REC_CORR
// or PATH_REC, G = 10 or 5, softsign or tanh_fast, and the launch bound 256 or 1024 that holds `threads`.
template <class Go>
auto fk_small_ladder(const LayerConst& hlc, int threads, Go&& go) {
    auto by_block = [&](auto norm, auto path, auto gt) {
        return threads <= 256 ? go(norm, path, gt, ITag<256>{}) : go(norm, path, gt, ITag<1024>{});
    };
    auto by_norm = [&](auto path, auto gt) {
        return hlc.norm == NORM_SOFTSIGN ? by_block(ITag<NORM_SOFTSIGN>{}, path, gt)
                                         : by_block(ITag<NORM_TANH_FAST>{}, path, gt);
    };
    auto by_g = [&](auto path) { return hlc.G == 10 ? by_norm(path, ITag<10>{}) : by_norm(path, ITag<5>{}); };
    return hlc.path == PATH_REC_CORR ? by_g(ITag<PATH_REC_CORR>{}) : by_g(ITag<PATH_REC>{});
}
// The Dual solve and the training loop on it (fk_small_fsens_supported): go(norm, gt, tab, e) with G = 10 or 5,
// softsign or tanh_fast, the tables or the reference formula, and two entries per lane or one.
template <class Go>
auto fk_fsens_ladder(const LayerConst& hlc, bool tab, bool two, Go&& go) {
    auto by_e = [&](auto norm, auto gt, auto tb) {
        return two ? go(norm, gt, tb, ITag<2>{}) : go(norm, gt, tb, ITag<1>{});
    };
    auto by_tab = [&](auto norm, auto gt) {
        return tab ? by_e(norm, gt, std::true_type{}) : by_e(norm, gt, std::false_type{});
    };
    auto by_norm = [&](auto gt) {
        return hlc.norm == NORM_SOFTSIGN ? by_tab(ITag<NORM_SOFTSIGN>{}, gt) : by_tab(ITag<NORM_TANH_FAST>{}, gt);
    };
    return hlc.G == 10 ? by_norm(ITag<10>{}) : by_norm(ITag<5>{});
}

}  // namespace kan
