// kan_train_body.inc — the loop of one replica (kan_train.hip's header comment): the body of
// kd_chain_train_lvsp_kernel and of kd_chain_train_lvsp_ens_kernel, included into both with the replica's
// ChainTrainArgs `a`, the layer constants `lcs` and the template parameters NORM, FN, PATH, FS in scope.  It
// reads no block index.  (Text, not a device function: the single-replica kernel then compiles to the code it
// had before the ensemble entry existed; as an inlined function its register allocation moved -- DESIGN §7.)
    constexpr int N = LvWaveShape::I, P = kLvP;
    extern __shared__ __attribute__((aligned(16))) unsigned char cv_raw[];
    LayerConst* lcl = reinterpret_cast<LayerConst*>(cv_raw);
    double* ps = reinterpret_cast<double*>(cv_raw + 2 * sizeof(LayerConst));
    double* tsl = ps + P;            // [cap]
    double* dtsl = tsl + a.cap;      // [cap]
    double* recl = dtsl + a.cap;     // [cap][7][N], then k1_0 [N] (stage_rec)
    double* sv = a.stage_rec ? recl + (a.cap * 7 + 1) * N : recl;   // saveat [n_save]
    double* dl = sv + a.n_save;      // u_save, then dl [n_save][N]
    double* svt = dl + a.n_save * N; // the test problem's saveat [n_save_test]
    double* ust = svt + a.n_save_test;   // its u_save [n_save_test][N]
    __shared__ LvSpLds S;
    __shared__ int64_t fo[2][4];     // the counters of wave 0's and wave 1's solve
    __shared__ double lossv;         // loss[it]
    S.fill_tableau();
    {
        const int nw = 2 * (int)(sizeof(LayerConst) / sizeof(int32_t));
        const int32_t* src = reinterpret_cast<const int32_t*>(lcs);
        int32_t* dst = reinterpret_cast<int32_t*>(cv_raw);
        stage_chain_consts(dst, src, nw, ps, a.p, P);
        for (int64_t i = threadIdx.x; i < a.n_save; i += blockDim.x) sv[i] = a.saveat[i];
        for (int64_t i = threadIdx.x; i < a.n_save_test; i += blockDim.x) svt[i] = a.saveat_test[i];
        if (threadIdx.x < 8) fo[threadIdx.x / 4][threadIdx.x % 4] = 0;
    }
    KAN_EXP_TABLE_LDS(tab);
    const Math<double> M{tab};
    const int lane = threadIdx.x & (kWave - 1);
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const bool has_test = a.n_save_test > 0 && a.loss_test != nullptr;
    double* const rec = a.stage_rec ? recl : a.rec;
    double* const rk1 = rec + a.cap * 7 * N;
    ChainAdjointArgs aa{};   // (rec, k1_0, ts, dts, nsteps and the outputs: lvsp_adjoint's own arguments)
    aa.t0 = a.t0;
    aa.tf = a.tf;
    aa.dt = a.dt;
    aa.abstol = a.abstol;
    aa.reltol = a.reltol;
    aa.dtmin = a.dtmin;
    aa.beta1 = a.beta1;
    aa.beta2 = a.beta2;
    aa.gamma = a.gamma;
    aa.qmin = a.qmin;
    aa.qmax = a.qmax;
    aa.qoldinit = a.qoldinit;
    aa.adaptive = a.adaptive;
    aa.maxiters = a.maxiters;
    aa.dl_du = dl;
    aa.stops = a.stops;
    aa.nstops = a.nstops;
    aa.jrows = a.jrows;
    aa.joff = a.joff;
    double bp1 = a.bp1, bp2 = a.bp2;
    int64_t done = 0;
    int reason = kTrainOk;
    for (int64_t it = 0; it <= a.n_iters; ++it) {
        if (it == a.n_iters && !(has_test && it > 0)) break;
        // ---- A: the solves at p_it (wave 0: training, dense output kept; wave 1: test) ----
        const bool tst = w == 1;
        if (w < 2 && (tst ? (has_test && it > 0) : it < a.n_iters)) {
            ChainSolveArgs fa{};
            fa.t0 = a.t0;
            fa.tf = tst ? a.tf_test : a.tf;
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
            fa.n_save = tst ? a.n_save_test : a.n_save;
            fa.cap = a.cap;
            fa.saveat = tst ? svt : sv;
            fa.u_save = tst ? ust : dl;
            fa.rec = tst ? nullptr : rec;
            fa.k1_0 = rk1;
            fa.ts = tsl;
            fa.dts = dtsl;
            fa.out = fo[tst ? 1 : 0];
            const int j = threadIdx.x & (kChainDim - 1);
            ChainModel<double, FN, PATH, FS> fm{M, lcl, 2, ps, nullptr, P, j, 0, lane < N, (int64_t)lane, (int64_t)N};
            onewg_tsit5<double, ChainModel<double, FN, PATH, FS>, true>(fm, a.u0, fa, nullptr);
            __threadfence_block();   // the wave's u_save (lanes < N wrote it) before every lane reads it
            if (tst) {
                const double lt = wave_mse<false>(ust, a.target_test, a.n_save_test * N, 0.0);
                if (lane == 0) a.loss_test[it - 1] = fo[1][3] == 0 ? lt : __longlong_as_double(0x7ff8000000000000LL);
            } else if (fo[0][3] == 0) {   // (lane 0's own store, read back by the wave)
                double lv = wave_mse<true>(dl, a.target, a.n_save * N, a.dl_scale);
                if (a.act_reg != 0.0) lv = l1_loss(lv, ps, P, a.act_reg);   // (λ = 0: not one operation more)
                if (lane == 0) {
                    a.loss[it] = lv;
                    lossv = lv;
                }
            }
        }
        __syncthreads();
        if (has_test && it > 0 && fo[1][3] != 0) {
            reason = kTrainTestMaxiters;
            break;
        }
        if (it == a.n_iters) break;
        if (fo[0][3] != 0) {
            reason = fo[0][3] == 2 ? kTrainDenseCapacity : kTrainForwardMaxiters;
            break;
        }
        if (!(::fabs(lossv) <= 1.7976931348623157e308)) {
            reason = kTrainLossNotFinite;
            break;
        }
        // ---- B: the InterpolatingAdjoint from the dense output just written ----
        double mu[kLvPL], l0, l1;
        int64_t res[4];
        lvsp_adjoint<NORM>(S, M, lcl, ps, aa, fo[0][0], rec, rk1, tsl, dtsl, mu, l0, l1, res);
        if (res[3] != 0) {
            reason = kTrainAdjointMaxiters;
            break;
        }
        // ---- C: records and Adam (wave 0: lane l holds the gradient entries l + 64 r) ----
        if (w == 0) {
            if (a.counts && lane == 0) {
                a.counts[4 * it] = fo[0][0];
                a.counts[4 * it + 1] = fo[0][1];
                a.counts[4 * it + 2] = res[0];
                a.counts[4 * it + 3] = res[1];
            }
            AdamArgs ad;
            ad.scale = 1.0;
            ad.beta1 = a.ab1;
            ad.beta2 = a.ab2;
            ad.omb1 = a.omb1;
            ad.omb2 = a.omb2;
            {   // (contraction off: 1 - βp must not fuse with the product that advanced βp below)
#pragma clang fp contract(off)
                ad.c1 = 1.0 - bp1;
                ad.c2 = 1.0 - bp2;
            }
            ad.eps = a.eps;
            ad.eta = a.eta;
#pragma unroll
            for (int r = 0; r < kLvPL; ++r) {
                const int q = lane + kWave * r;
                if (q < P) {
                    const double x = ps[q];
                    double gq = mu[r];
                    // ∂(λ·Σ|p|)/∂p_q = λ·sgn(p_q), sgn(0) = 0: one rounded add (λ = 0: none, a -0.0 stays -0.0)
                    if (a.act_reg != 0.0) gq = __dadd_rn(gq, x > 0.0 ? a.act_reg : (x < 0.0 ? -a.act_reg : 0.0));
                    if (a.grad) a.grad[it * P + q] = gq;
                    if (a.p_before) a.p_before[it * P + q] = x;
                    double mq = a.m[q], vq = a.v[q];
                    const double xn = adam_entry<double>(x, mq, vq, gq, ad);
                    a.m[q] = mq;
                    a.v[q] = vq;
                    a.p[q] = xn;
                    ps[q] = xn;
                }
            }
        }
        __syncthreads();   // p_{it+1} in LDS; every wave is done with dl, the dense output and the rows
        {   // the rounded products Python's `bp *= β` forms
#pragma clang fp contract(off)
            bp1 = bp1 * a.ab1;
            bp2 = bp2 * a.ab2;
        }
        done = it + 1;
    }
    if (threadIdx.x == 0) {
        a.out[0] = done;
        a.out[1] = reason;
    }
