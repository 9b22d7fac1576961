// kan_train_wg_body.inc -- the body of kd_chain_train_wg_kernel and kd_chain_train_wg_ens_kernel (kan_train_wg.hip),
// included into both as text (as kan_train_body.inc is into the Lotka-Volterra pair), so the single-replica
// kernel's code does not depend on its ensemble twin.  In scope: the template parameters FN, PATH, FS, ADJ, WN, the
// kernel arguments lcs, nl, P, and `a`, this workgroup's ChainTrainArgs (the kernel argument, or the workgroup's copy
// of args[blockIdx.x]).  Nothing here reads a block index.
    extern __shared__ __attribute__((aligned(16))) unsigned char tw_raw[];
    __shared__ double red[kChainBlock / kWave];
    __shared__ int64_t fo[12];
    __shared__ double lossv;
    const int64_t n = a.N * a.B;
    const int64_t work = ADJ == kWgWide ? (int64_t)WideModel<double, WN>::kEnd : (int64_t)(blockDim.x / kChainDim) * P;
    const TrainWgCarve c = train_wg_carve(P, work, a.cap, a.n_save, a.n_save_test, n, a.dl_lds, a.stage_rec);
    double* const base = reinterpret_cast<double*>(tw_raw + nl * sizeof(LayerConst));
    TrainWgPtrs L;
    L.lcl = (KAN_LDS const LayerConst*)reinterpret_cast<const LayerConst*>(tw_raw);
    L.ps = (KAN_LDS double*)(base + c.ps);
    L.work = (KAN_LDS double*)(base + c.work);
    L.mu = (KAN_LDS double*)(base + c.mu);
    L.km = (KAN_LDS double*)(base + c.km);
    L.gl = (KAN_LDS double*)(base + c.gl);
    L.tsl = (KAN_LDS double*)(base + c.tsl);
    L.dtsl = (KAN_LDS double*)(base + c.dtsl);
    L.sv = (KAN_LDS double*)(base + c.sv);
    L.svt = (KAN_LDS double*)(base + c.svt);
    L.rec = a.rec;
    L.rk1 = a.rec + a.cap * 7 * n;
    L.dl = a.dl_lds ? base + c.dl : L.rk1 + n;
    L.ust = a.dl_lds ? base + c.ust : L.rk1 + n + a.n_save * n;
    L.recl = (KAN_LDS double*)(base + c.recl);
    L.red = (KAN_LDS double*)red;
    L.fo = (KAN_LDS int64_t*)fo;
    L.lossv = (KAN_LDS double*)&lossv;
    L.nl = nl;
    L.P = P;
    {
        const int nw = nl * (int)(sizeof(LayerConst) / sizeof(int32_t));
        const int32_t* src = reinterpret_cast<const int32_t*>(lcs);
        int32_t* dst = reinterpret_cast<int32_t*>(tw_raw);
        stage_chain_consts(dst, src, nw, base + c.ps, a.p, P);
        for (int64_t i = threadIdx.x; i < a.n_save; i += blockDim.x) L.sv[i] = a.saveat[i];
        for (int64_t i = threadIdx.x; i < a.n_save_test; i += blockDim.x) L.svt[i] = a.saveat_test[i];
        if (threadIdx.x < 12) fo[threadIdx.x] = 0;
    }
    KAN_EXP_TABLE_LDS(tab);   // (its barrier also publishes the constants, ps, the saveat lists and fo)
    L.tab = (KAN_LDS const double*)tab;
    const bool has_test = a.n_save_test > 0 && a.loss_test != nullptr;
    double bp1 = a.bp1, bp2 = a.bp2;
    int64_t done = 0;
    int reason = kTrainOk;
    for (int64_t it = 0; it <= a.n_iters; ++it) {
        const bool tst = has_test && it > 0;
        if (it == a.n_iters && !tst) break;
        // ---- A: the solves at p_it, the loss and its cotangent ----
        if (it < a.n_iters) {
            wg_forward<FN, PATH, FS>(a, L, false);
            __syncthreads();   // u_save, the dense output, ts / dts and the counters, to every wave
            if (fo[3] == 0) wg_loss(a, L, it);
        }
        if (tst) {
            wg_forward<FN, PATH, FS>(a, L, true);
            __syncthreads();
            wg_test_loss(a, L, it);
        }
        __syncthreads();
        if (tst && fo[7] != 0) {
            reason = kTrainTestMaxiters;
            break;
        }
        if (it == a.n_iters) break;
        if (fo[3] != 0) {
            reason = fo[3] == 2 ? kTrainDenseCapacity : kTrainForwardMaxiters;
            break;
        }
        if (!(::fabs(lossv) <= 1.7976931348623157e308)) {
            reason = kTrainLossNotFinite;
            break;
        }
        // ---- B: the InterpolatingAdjoint from the dense output just written ----
        wg_adjoint<ADJ, WN, FN, PATH, FS>(a, L);
        __syncthreads();   // the gradient and the adjoint's counters
        if (fo[11] != 0) {
            reason = kTrainAdjointMaxiters;
            break;
        }
        // ---- C: records and Adam ----
        wg_adam(a, L, it, bp1, bp2);
        __syncthreads();   // p_{it+1} in LDS; every wave is done with dl, the gradient and the counters
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
