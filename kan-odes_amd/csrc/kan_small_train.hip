// kan_small_train.hip — K whole training iterations of the Fisher-KPP source-term problem on the forward-mode
// gradient in ONE launch (gfx950).
//
// The reference's Fisher-KPP / Allen-Cahn source drivers (PDE examples/Fisher-KPP_Source.jl:194-213) are, per
// iteration, Zygote.gradient(loss, p) -- ForwardDiffSensitivity at these sizes --, Flux's Adam update and loss(p)
// again at the updated parameters.  The Dual solve was one workgroup already (fk_small_fsens_kernel) and carries
// everything a gradient needs; u0, tspan, saveat, the target and the options are the same every iteration, only p
// and the Adam moments change, so here the whole loop stays on the device.
//
// One workgroup of G + 2 waves with the layout of fk_small_fsens_kernel (wave 0 the values, wave 1 + k the partial
// S_k, E entries per lane).  Per iteration `it`:
//   A  (TAB) every thread: the PP_PHI, PP_DPHI and PP_SWISH tables at p_it, built straight into the LDS tables by
//      pp_build_block over virtual blocks of 256 threads (the text of fk_pp_build_kernel: the launch's bits)
//   B  (TEST: the kernel of a launch with a test problem; it > 0) the plain solve over (t0, tf_test) at
//      p_it = p_{(it-1)+1}: onewg_tsit5 with FkSmallModel on waves 0..B-1 (fk_small_tsit5_kernel's arithmetic,
//      PP_PHI from A) -> loss_test[it-1] and its counts; the last one runs after the loop behind a PP_PHI build
//   C  the Dual solve at p_it (fk_small_fsens_body), whose saveat stops are not stored but
//   D  accumulated (each lane's own column: LDS, global memory at two entries per lane): wave 0 forms
//      d = u - X[j], lacc = fma(d, d, lacc) and the row dl = d·scale in LDS; after a
//      barrier partial wave k takes gacc = fma(dl[e], S_k[e], gacc) per entry (the row alternates by the stop's
//      parity, so one barrier per stop)
//   E  loss[it] = wave_sum(lacc_lo + lacc_hi)/cnt, g_k = wave_sum(gacc_lo + gacc_hi): per lane in saveat order,
//      then the wave butterfly; a solve at maxiters or a non-finite loss stops the loop before the update
//   F  wave 0: the optional records, then Adam on lanes k < P (adam_entry: the statement of adam_step_kernel) -> p
//      (global and the LDS copy), m, v; βp1, βp2 (LDS: a register pair per thread is what this kernel does not have)
//      advance by one rounded product; a barrier closes the iteration.
// The parameters are read from their LDS copy throughout (the table build, the reference formula of points off
// the tables): p changes inside the kernel, and global p is written for the host only.
#include "kan_small_fsens.hpp"
#include "kan_pp_build.hpp"

namespace kan {

namespace {

// The rows that follow the Dual solve's own LDS (fk_small_fsens_lds_doubles), as offsets in doubles.  The table
// build's scratch and the test solve's u_save are live only while the Dual solve's rows (everything after the
// tables) are dead, and overlay them where they fit.  At two entries per lane the accumulators live in global memory
// (ChainTrainArgs::rec): with the tables and the parked state the Dual solve alone takes 144 KB.
struct FkTrainLds {
    size_t ps, acc, dl, ust, bQ, bT, bC, bG, scr, total;
};
__host__ __device__ inline FkTrainLds fk_train_lds(bool tab, int ni, int G, bool two, int64_t n,
                                                   int64_t n_save_test) {
    const size_t W = (two ? 2 : 1) * kWave;
    FkTrainLds o{};
    const size_t rows = tab ? 3 * (size_t)kPPCoef * (size_t)ni : 0;   // where the Dual solve's rows begin
    size_t q = fk_small_fsens_lds_doubles(tab, ni, G, two);
    const size_t rows_end = q;
    auto take = [&](size_t cnt) {
        const size_t at = q;
        q += (cnt + 1) & ~(size_t)1;   // (16-byte granules)
        return at;
    };
    o.ps = take(kMaxGrid + 1);                   // the parameters C_0..C_{G-1}, W
    o.acc = two ? 0 : take((size_t)(G + 2) * W); // lacc (wave 0) / gacc (wave 1 + k), each lane's own column
    o.dl = take(2 * W);                          // the cotangent row of a stop, by the stop's parity
    if (tab) {                                   // the table build's constants
        o.bQ = take(kPPCoef * kPPCoef);
        o.bT = take(kPPEvals);
        o.bC = take(kMaxGrid + 1);
        o.bG = take(kMaxGrid);
    }
    const size_t nscr = tab ? (size_t)kPPBuildScratch * (((G + 2) * kWave) / kBlock) : 0;
    const size_t nust = ((size_t)n_save_test * n + 1) & ~(size_t)1;
    if (rows + nscr + nust <= rows_end) {        // overlaid on the Dual solve's rows
        o.scr = rows;
        o.ust = rows + nscr;
    } else {
        o.scr = take(nscr);
        o.ust = take(nust);
    }
    o.total = q;
    return o;
}

// Σ_i (us[i] - X[i])² / cnt over the calling wave (kan_train.hip's wave_mse: lane l sums its terms l, l + 64, .. in
// order, then the wave butterfly)
__device__ __forceinline__ double wave_mse_lds(const double* __restrict__ us, const double* __restrict__ X,
                                               int64_t cnt) {
    const int lane = threadIdx.x & (kWave - 1);
    double s = 0.0;
    for (int64_t i = lane; i < cnt; i += kWave) {
        const double d = __dsub_rn(us[i], X[i]);
        s = ::fma(d, d, s);
    }
    return __ddiv_rn(wave_sum(s), (double)cnt);
}

// (the loop of one replica: the body of both entry kernels below; it reads no block index)
template <int NORM, int GT, bool TAB, int E, bool TEST>
__device__ __forceinline__ void fk_small_train_body(const LayerConst* __restrict__ lcp,
                                                    const PPConst* __restrict__ pcp, const FkSmallArgs& s, int64_t B,
                                                    const ChainTrainArgs& a) {
    constexpr int P = GT + 1, W = E * kWave;
    extern __shared__ double2 tl[];
    __shared__ double red[kFsensMaxWaves];
    __shared__ int64_t fo[2][4];     // the counters of the Dual solve and of the test solve
    __shared__ double lossv;         // loss[it]
    __shared__ double gl[P];         // the gradient of iteration it
    __shared__ double bpl[2];        // the running powers βp1, βp2
    const int tid = threadIdx.x;
    const int64_t n = (int64_t)s.Nx * B;
    static_assert(TAB || !TEST, "the logged-loss solve reads the PP_PHI table");
    constexpr bool has_test = TEST;   // (phase B is compiled into the kernels of a launch with a test problem only)
    const int64_t nst = has_test ? a.n_save_test : 0;
    const FkTrainLds o = fk_train_lds(TAB, s.ni, GT, E == 2, n, nst);
    double* const base = reinterpret_cast<double*>(tl);
    double* const ps = base + o.ps;
    double* const dlr = base + o.dl;
    double* const ust = base + o.ust;   // the test solve's u_save
    // (the targets are read where they lie: the kernel never writes them)
    const double* __restrict__ const X = a.target;
    const double* __restrict__ const Xt = a.target_test;
    if (tid <= kMaxGrid) ps[tid] = tid < P ? a.p[tid] : 0.0;
    if (tid < 8) fo[tid / 4][tid % 4] = 0;
    if (tid < 2) bpl[tid] = tid == 0 ? a.bp1 : a.bp2;
    if constexpr (TAB) {   // the build's constants (fk_pp_build_kernel's first round of loads)
        const PPConst& pc = *pcp;
        double* sQ = base + o.bQ;
        double* sT = base + o.bT;
        double* sG = base + o.bG;
        if (tid < kPPCoef * kPPCoef) sQ[tid] = (&pc.Q[0][0])[tid];
        if (tid < kPPEvals) sT[tid] = tid < kPPCoef ? pc.xi[tid] : pc.tchk[tid - kPPCoef];
        if (tid < GT) sG[tid] = (double)lcp->grid[tid];
    }
    KAN_EXP_TABLE_LDS(tab);   // (its barrier also publishes the rows above)
    const Math<double> M{tab};
    // A: nfn tables (PP_PHI, PP_DPHI, PP_SWISH in slot order) at the parameters in ps, into tl
    auto build = [&](int nfn, int tid, int ni, const LayerConst& lc, const PPConst& pc) {
        if constexpr (TAB) {
            double* sC = base + o.bC;
            if (tid <= GT) sC[tid] = ps[tid];
            const int nvb = (int)blockDim.x / kBlock;   // virtual blocks worked off per pass
            const int vb = tid / kBlock, vt = tid - vb * kBlock;
            const bool grp = vb < nvb;
            double* scr = base + o.scr + (size_t)(grp ? vb : 0) * kPPBuildScratch;
            const PPBuildLds L{base + o.bQ, base + o.bT, sC, base + o.bG, scr};
            const int nb = ni / kPPPerBlock, tot = nfn * nb;
            for (int v0 = 0; v0 < tot; v0 += nvb) {
                const int v = v0 + vb;
                const bool on = grp && v < tot;
                const int fn = on ? v / nb : 0, blk = on ? v - fn * nb : 0;
                if (on && vt < kPPPerBlock) pp_build_bad(scr)[vt] = 0;
                __syncthreads();   // sC, bad
                pp_build_block(M, lc, pc, L, blk, fn, vt, on, base + (size_t)fn * kPPCoef * ni);
                __syncthreads();   // the pass's tables; its scratch is free
            }
        }
    };
    ChainSolveArgs fa{};
    fa.t0 = a.t0;
    fa.tf = a.tf;
    fa.dt = a.dt;
    fa.abstol = a.abstol;
    fa.reltol = a.reltol;
    fa.dtmin = a.dtmin;
    fa.beta1 = a.beta1;
    fa.beta2 = a.beta2;
    fa.gamma = a.gamma;
    fa.qmin = a.qmin;
    fa.qmax = a.qmax;
    fa.qoldinit = a.qoldinit;
    fa.adaptive = a.adaptive;
    fa.maxiters = a.maxiters;
    fa.n_save = a.n_save;
    fa.saveat = a.saveat;
    fa.out = fo[0];
    // D: a saveat stop of the Dual solve
    double* accl = nullptr;   // this lane's column of the accumulators (+ kWave: its upper entry), set per iteration
    int wv = 0;               // this thread's wave, likewise
    auto stop = [&](int64_t si, const double (&v)[E], const bool (&act)[E], const int (&e)[E]) {
        double* row = dlr + (si & 1) * W;
        if (wv == 0) {
#pragma unroll
            for (int h = 0; h < E; ++h) {
                if (!act[h]) continue;
                const double d = __dsub_rn(v[h], X[si * n + e[h]]);
                accl[h * kWave] = ::fma(d, d, accl[h * kWave]);
                row[e[h]] = __dmul_rn(d, a.dl_scale);
            }
        }
        __syncthreads();
        if (wv > 0) {
#pragma unroll
            for (int h = 0; h < E; ++h)
                if (act[h]) accl[h * kWave] = ::fma(row[e[h]], v[h], accl[h * kWave]);
        }
    };
    int64_t done = 0;
    int reason = kTrainOk;
    for (int64_t it = 0; it <= a.n_iters; ++it) {
        const bool last = it == a.n_iters;
        if (last && !(has_test && it > 0)) break;
        // (opaque per iteration: what the phases derive from the lane, the field's shape and the layer's constants is
        // loop-invariant, and hoisted out of the iteration loop it would stay live across every phase, in registers
        // this kernel does not have)
        FkSmallArgs si = s;
        int tdi = tid;
        const LayerConst* lci = lcp;
        const PPConst* pci = pcp;
        asm volatile(""
                     : "+s"(si.Nx), "+s"(si.ni), "+s"(si.inv_w), "+s"(si.x0), "+s"(si.cd), "+s"(si.co), "+v"(tdi),
                       "+s"(lci), "+s"(pci));
        const LayerConst& lc = *lci;
        const int w = tdi / kWave, l = tdi & (kWave - 1);   // (of the iteration's opaque index, as every phase's)
        // (likewise what the solves derive from their options: t0 + ε, tf - t0, the norms' counts)
        ChainSolveArgs fi = fa;
        int64_t Bi = B;
        asm volatile(""
                     : "+s"(fi.t0), "+s"(fi.tf), "+s"(fi.dt), "+s"(fi.abstol), "+s"(fi.reltol), "+s"(fi.dtmin),
                       "+s"(fi.beta1), "+s"(fi.beta2), "+s"(fi.gamma), "+s"(fi.qmin), "+s"(fi.qmax), "+s"(fi.qoldinit),
                       "+s"(Bi));
        build(last ? 1 : 3, tdi, si.ni, lc, *pci);
        // ---- B: the test-loss solve of iteration it - 1 (the plain solve at p_it) ----
        if constexpr (TEST) {
            if (it > 0) {
                ChainSolveArgs ta = fi;
                ta.tf = a.tf_test;
                ta.n_save = a.n_save_test;
                ta.saveat = a.saveat_test;
                ta.u_save = ust;
                ta.out = fo[1];
                auto m = fk_small_model<NORM, PATH_REC, GT>(M, lc, ps, tl, nullptr, si, Bi, nullptr, tdi);
                onewg_tsit5<double>(m, a.u0, ta, red);
                __syncthreads();   // u_save and the counters
                if (w == 0) {
                    const double lt = wave_mse_lds(ust, Xt, a.n_save_test * n);
                    if (l == 0) {
                        a.loss_test[it - 1] = fo[1][3] == 0 ? lt : __longlong_as_double(0x7ff8000000000000LL);
                        if (a.counts) {   // (the record of iteration it - 1: its logged-loss solve ran just now)
                            a.counts[4 * (it - 1) + 2] = fo[1][0];
                            a.counts[4 * (it - 1) + 3] = fo[1][1];
                        }
                    }
                }
                if (__builtin_amdgcn_readfirstlane((int)fo[1][3]) != 0) {   // (uniform, and known to be)
                    reason = kTrainTestMaxiters;
                    break;
                }
            }
        }
        if (last) break;
        // ---- C, D: the Dual solve at p_it, its stops accumulated ----
        accl = (E > 1 ? a.rec : base + o.acc) + (size_t)w * W + l;
        wv = w;
#pragma unroll
        for (int h = 0; h < E; ++h) accl[h * kWave] = 0.0;
        fk_small_fsens_body<NORM, GT, TAB, E>(M, lc, ps, tl, red, si, a.u0, Bi, fi, stop, tdi);
        // ---- E: loss, gradient and the stop checks ----
        {
            double t = accl[0];
            if constexpr (E > 1) t = t + accl[kWave];
            t = wave_sum(t);
            if (l == 0) {
                if (w == 0) lossv = __ddiv_rn(t, (double)(a.n_save * si.Nx * Bi));
                else gl[w - 1] = t;
            }
        }
        __syncthreads();   // lossv, gl and the solve's counters
        if (__builtin_amdgcn_readfirstlane((int)fo[0][3]) != 0) {
            reason = kTrainForwardMaxiters;
            break;
        }
        if (tdi == 0) a.loss[it] = lossv;
        if (__builtin_amdgcn_readfirstlane((int)!(::fabs(lossv) <= 1.7976931348623157e308))) {
            reason = kTrainLossNotFinite;
            break;
        }
        // ---- F: records and Adam (wave 0: lane k holds parameter k) ----
        if (w == 0) {
            if (a.counts && l == 0) {
                a.counts[4 * it] = fo[0][0];
                a.counts[4 * it + 1] = fo[0][1];
            }
            AdamArgs ad;
            ad.scale = 1.0;
            ad.beta1 = a.ab1;
            ad.beta2 = a.ab2;
            ad.omb1 = a.omb1;
            ad.omb2 = a.omb2;
            {   // (contraction off: 1 - βp must not fuse with the product that advanced βp below)
#pragma clang fp contract(off)
                ad.c1 = 1.0 - bpl[0];
                ad.c2 = 1.0 - bpl[1];
            }
            ad.eps = a.eps;
            ad.eta = a.eta;
            if (l < P) {
                double *pm = a.m, *pv = a.v, *pp = a.p, *pg = a.grad, *pb = a.p_before;
                // (opaque: no lane address of theirs is kept across the solve)
                asm volatile("" : "+s"(pm), "+s"(pv), "+s"(pp), "+s"(pg), "+s"(pb));
                const double x = ps[l], g = gl[l];
                if (pg) pg[it * P + l] = g;
                if (pb) pb[it * P + l] = x;
                double mq = pm[l], vq = pv[l];
                const double xn = adam_entry<double>(x, mq, vq, g, ad);
                pm[l] = mq;
                pv[l] = vq;
                pp[l] = xn;
                ps[l] = xn;
            }
        }
        if (tdi < 2) {   // the rounded products Python's `bp *= β` forms (wave 0 has read them: program order)
#pragma clang fp contract(off)
            bpl[tdi] = bpl[tdi] * (tdi == 0 ? a.ab1 : a.ab2);
        }
        __syncthreads();   // p_{it+1} in LDS; every wave is done with the slots, the rows and the counters
        done = it + 1;
    }
    if (tid == 0) {
        a.out[0] = done;
        a.out[1] = reason;
    }
}

template <int NORM, int GT, bool TAB, int E, bool TEST>
__global__ void __launch_bounds__((GT + 2) * kWave)
fk_small_train_kernel(const LayerConst* __restrict__ lcp, const PPConst* __restrict__ pcp, FkSmallArgs s, int64_t B,
                      ChainTrainArgs a) {
    fk_small_train_body<NORM, GT, TAB, E, TEST>(lcp, pcp, s, B, a);
}

// The ensemble entry: workgroup r runs the loop on args[r] (its own p, m, v, Adam scalars, records, accumulator
// block and status words; the tables are built into each workgroup's own LDS).  The workgroups share nothing they
// write and never wait for each other.
template <int NORM, int GT, bool TAB, int E, bool TEST>
__global__ void __launch_bounds__((GT + 2) * kWave)
fk_small_train_ens_kernel(const LayerConst* __restrict__ lcp, const PPConst* __restrict__ pcp, FkSmallArgs s,
                          int64_t B, const ChainTrainArgs* __restrict__ args) {
    const ChainTrainArgs a = args[blockIdx.x];
    fk_small_train_body<NORM, GT, TAB, E, TEST>(lcp, pcp, s, B, a);
}
}  // namespace

bool fk_small_train_supported(const LayerConst& hlc, const PPConst& hpc, bool tab, int Nx, int64_t B, int wide,
                              bool with_test) {
    if (!fk_small_fsens_supported(hlc, Nx, B, wide)) return false;
    // the logged-loss solve: fk_small_tsit5_kernel's shapes, one trajectory per wave of this block
    return !with_test || (tab && fk_small_supported(hlc, hpc, Nx, B) && B <= hlc.G + 2);
}

// args == nullptr: the single-replica kernel on `a`; else the ensemble kernel, one workgroup per struct of the device
// array args [n_rep] (a: the host copy of any one of them -- they agree in every field read here)
static hipError_t launch_fk_train(const LayerConst& hlc, const PPConst& hpc, bool tab, const LayerConst* lc,
                                  const PPConst* pc, const FkSmallArgs& s, int64_t B, const ChainTrainArgs& a,
                                  const ChainTrainArgs* args, int64_t n_rep, int wide, hipStream_t st) {
    const bool with_test = a.n_save_test > 0 && a.loss_test != nullptr;
    if (!fk_small_train_supported(hlc, hpc, tab, s.Nx, B, wide, with_test) ||
        (tab && (!hpc.enabled || s.ni != hpc.ni || hpc.ni % kPPPerBlock || !pc)) || a.n_iters < 1 || a.n_save < 1 ||
        a.n_save_test < 0 || (args && (n_rep < 1 || n_rep > kTrainMaxReplicas)))
        return hipErrorNotSupported;
    const int threads = (hlc.G + 2) * kWave;
    const bool two = wide == 2 || (int64_t)s.Nx * B > kWave;   // entries per lane (launch_fk_small_fsens's rule)
    const size_t lds = sizeof(double) * fk_train_lds(tab, hpc.ni, hlc.G, two, (int64_t)s.Nx * B, a.n_save_test).total;
    if (lds > 150 * 1024 || (two && !a.rec)) return hipErrorNotSupported;
    // test: the kernel holds the logged-loss solve (with the tables only: fk_small_train_supported)
    auto go = [&](auto norm, auto gt, auto tb, auto e, auto test) {
        const void* fn = args ? reinterpret_cast<const void*>(&fk_small_train_ens_kernel<norm(), gt(), tb(), e(), test()>)
                              : reinterpret_cast<const void*>(&fk_small_train_kernel<norm(), gt(), tb(), e(), test()>);
        const hipError_t err = ensure_dynamic_lds(fn, lds);
        if (err != hipSuccess) return err;
        if (args)
            hipLaunchKernelGGL((fk_small_train_ens_kernel<norm(), gt(), tb(), e(), test()>), dim3((unsigned)n_rep),
                               dim3(threads), lds, st, lc, pc, s, B, args);
        else
            hipLaunchKernelGGL((fk_small_train_kernel<norm(), gt(), tb(), e(), test()>), dim3(1), dim3(threads), lds, st,
                               lc, pc, s, B, a);
        return hipGetLastError();
    };
    return fk_fsens_ladder(hlc, tab, two, [&](auto norm, auto gt, auto tb, auto e) {
        return tb() && with_test ? go(norm, gt, tb, e, tb) : go(norm, gt, tb, e, std::false_type{});
    });
}

hipError_t launch_fk_small_train(const LayerConst& hlc, const PPConst& hpc, bool tab, const LayerConst* lc,
                                 const PPConst* pc, const FkSmallArgs& s, int64_t B, const ChainTrainArgs& a, int wide,
                                 hipStream_t st) {
    return launch_fk_train(hlc, hpc, tab, lc, pc, s, B, a, nullptr, 1, wide, st);
}

hipError_t launch_fk_small_train_ensemble(const LayerConst& hlc, const PPConst& hpc, bool tab, const LayerConst* lc,
                                          const PPConst* pc, const FkSmallArgs& s, int64_t B, const ChainTrainArgs& a,
                                          const ChainTrainArgs* args, int64_t n_rep, int wide, hipStream_t st) {
    return args ? launch_fk_train(hlc, hpc, tab, lc, pc, s, B, a, args, n_rep, wide, st) : hipErrorNotSupported;
}

}  // namespace kan
