// kan_train_wg_adjoint.inc -- the body of phase B (kan_train_wg_phases.hpp's wg_adjoint), included as text into every
// function that runs it, so wg_adjoint's code does not depend on the others: wg_adjoint itself, and
// kan_traj_grad.hip's traj_adjoint, which also writes dL/du0.  In scope: the template parameters ADJ, WN, FN, PATH,
// FS, the arguments `a` (ChainTrainArgs) and `L` (TrainWgPtrs), and the macro KAN_WG_ADJOINT_DU0: empty (du0 stays
// null), or a statement that sets aa.du0.
    ChainAdjointArgs aa{};
    aa.t0 = wg_uniform(a.t0);
    aa.tf = wg_uniform(a.tf);
    aa.dt = wg_uniform(a.dt);
    aa.abstol = wg_uniform(a.abstol);
    aa.reltol = wg_uniform(a.reltol);
    aa.dtmin = wg_uniform(a.dtmin);
    aa.beta1 = wg_uniform(a.beta1);
    aa.beta2 = wg_uniform(a.beta2);
    aa.gamma = wg_uniform(a.gamma);
    aa.qmin = wg_uniform(a.qmin);
    aa.qmax = wg_uniform(a.qmax);
    aa.qoldinit = wg_uniform(a.qoldinit);
    aa.adaptive = wg_uniform(a.adaptive);
    aa.maxiters = wg_uniform(a.maxiters);
    aa.rec = wg_uniform(L.rec);
    aa.k1_0 = wg_uniform(L.rk1);
    aa.ts = (const double*)wg_uniform(L.tsl);
    aa.dts = (const double*)wg_uniform(L.dtsl);
    aa.nsteps = wg_uniform(L.fo[0]);
    aa.dl_du = wg_uniform(L.dl);
    aa.stops = wg_uniform(a.stops);
    aa.nstops = wg_uniform(a.nstops);
    aa.jrows = wg_uniform(a.jrows);
    aa.joff = wg_uniform(a.joff);
    KAN_WG_ADJOINT_DU0
    aa.dp = (double*)wg_uniform(L.gl);
    aa.out = (int64_t*)wg_uniform(L.fo) + 8;
    const Math<double> M{(const double*)wg_uniform(L.tab)};
    double* const mu = (double*)wg_uniform(L.mu);
    double* const km = (double*)wg_uniform(L.km);
    double* const work = (double*)wg_uniform(L.work);
    const double* const tsl = (const double*)wg_uniform(L.tsl);
    const double* const dtsl = (const double*)wg_uniform(L.dtsl);
    const LayerConst* const lcl = (const LayerConst*)wg_uniform(L.lcl);
    const double* const ps = (const double*)wg_uniform(L.ps);
    double* const red = (double*)wg_uniform(L.red);
    const int64_t B = wg_uniform(a.B);
    const int nl = wg_uniform(L.nl), stage_rec = wg_uniform(a.stage_rec);
    const int N = wg_uniform((int)a.N), P = wg_uniform(L.P);
    if constexpr (ADJ == kWgWide) {
        for (int i = threadIdx.x; i < WideModel<double, WN>::kEnd + 9 * P; i += blockDim.x) work[i] = 0.0;
        __syncthreads();
        double* recl = nullptr;
        if (stage_rec) {
            recl = (double*)wg_uniform(L.recl);
            onewg_stage_rec<double>(recl, aa, N);
        }
        WideModel<double, WN> m{M, lcl, ps, work, P, (int)threadIdx.x < N, (int64_t)threadIdx.x, (int64_t)N};
        onewg_adjoint<double>(m, aa, mu, km, tsl, dtsl, red, recl);
    } else {
        const int NG = blockDim.x / kChainDim;
        const int NGa = B < NG ? (int)B : NG;   // groups holding a trajectory
        for (int i = threadIdx.x; i < NG * P + 9 * P; i += blockDim.x) work[i] = 0.0;
        __syncthreads();
        const int j = threadIdx.x & (kChainDim - 1);
        const int64_t col = threadIdx.x / kChainDim;
        ChainModel<double, FN, PATH, FS> m{M, lcl, nl, ps, work, P, j, NGa, col < B && j < N, (int64_t)N * col + j,
                                           (int64_t)N * B};
        onewg_adjoint<double>(m, aa, mu, km, tsl, dtsl, red);
    }
