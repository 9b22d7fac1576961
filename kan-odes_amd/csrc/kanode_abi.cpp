// kanode_abi.cpp — the C-ABI (include/kanode.h) over the HIP kernels: the handle's life, its options and getters.
//
// Host-side responsibilities: validate the spec exactly as the reference ctor
// would accept it (kdense.jl:20-68), precompute the per-layer constants the
// kernels read (knots with Julia LinRange semantics, Float32 1/h, recurrence
// constants), own the device workspaces, and dispatch each layer to its kernel.
// No C++ exception crosses the ABI: every entry point returns a kanode_status.
//
// The handle itself is kanode_handle.hpp; the evaluation paths (RHS, VJP, stages) are kanode_eval.cpp, the
// one-launch steps / solves / adjoints kanode_fused.cpp, the training-loop launches kanode_train_launch.cpp.
#include "kanode.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>

#include "kanode_handle.hpp"

namespace {

// Julia LinRange{Float32}(a, b, G)[j] = Float32((1-t)*a + t*b), t = j/(G-1) in Float64.
void knots_linrange(float lo, float hi, int G, float* out) {
    const double a = (double)lo, b = (double)hi;
    for (int j = 0; j < G; ++j) {
        const double t = (double)j / (double)(G - 1);
        out[j] = (float)((1.0 - t) * a + t * b);
    }
}

bool norm_range(int norm, double& lo, double& hi) {
    switch (norm) {
    case KANODE_NORM_TANH_FAST:
    case KANODE_NORM_TANH:
    case KANODE_NORM_SOFTSIGN: lo = -1.0; hi = 1.0; return true;
    case KANODE_NORM_SIGMOID:
    case KANODE_NORM_SIGMOID_FAST: lo = 0.0; hi = 1.0; return true;
    default: return false;   // identity: unbounded
    }
}

// Host-side layer constants (see kan_device.hpp for the recurrence).
kanode_status make_layer_const(kanode_handle* h, const kanode_layer_spec& s, int dtype, int64_t p_off,
                               LayerConst& lc) {
    std::memset(&lc, 0, sizeof(lc));
    if (s.in_dims < 1 || s.out_dims < 1)
        return fail(h, KANODE_ERR_INVALID_ARG, "in_dims and out_dims must be >= 1");
    if (s.grid_len < 2 || s.grid_len > KANODE_MAX_GRID)
        return fail(h, KANODE_ERR_UNSUPPORTED, "grid_len must be in [2, " + std::to_string(KANODE_MAX_GRID) + "]");
    if (s.normalizer < 0 || s.normalizer > KANODE_NORM_IDENTITY)
        return fail(h, KANODE_ERR_INVALID_ARG, "unknown normalizer");
    if (s.basis < 0 || s.basis > KANODE_BASIS_IQF) return fail(h, KANODE_ERR_INVALID_ARG, "unknown basis");
    if (!(s.grid_hi > s.grid_lo)) return fail(h, KANODE_ERR_INVALID_ARG, "grid_lims must satisfy lo < hi");
    lc.I = s.in_dims;
    lc.O = s.out_dims;
    lc.G = s.grid_len;
    lc.norm = s.normalizer;
    lc.basis = s.basis;
    lc.use_base = s.use_base_act ? 1 : 0;
    lc.iqf_quirk = s.iqf_reference_quirk ? 1 : 0;
    lc.p_off = p_off;
    lc.w_off = p_off + (int64_t)lc.O * lc.G * lc.I;
    knots_linrange(s.grid_lo, s.grid_hi, lc.G, lc.grid);
    // (volatile keeps 1/h a Float32 division: the compiler may not fold it through a wider type)
    volatile float den = s.denominator > 0.f ? s.denominator : (float)(2.0 / (double)(lc.G - 1));
    volatile float one = 1.0f;
    lc.invh = one / den;   // Float32 1/h (utils.jl:9)
    const double sd = (double)lc.invh;
    lc.g0 = (double)lc.grid[0];
    lc.s = sd;
    lc.gs = -lc.g0 * sd;
    lc.delta = ((double)s.grid_hi - (double)s.grid_lo) * sd / (double)(lc.G - 1);
    lc.unit_delta = lc.delta == 1.0 ? 1 : 0;
    // the knot-rounding correction exp(2·z0·e_j) is expanded around the centre of
    // 2·z0 ∈ [2 z_lo, 2 z_hi] over the normalizer's range
    double nlo = -1.0, nhi = 1.0;
    const bool bounded = norm_range(lc.norm, nlo, nhi);
    const double zlo = (nlo - lc.g0) * sd, zhi = (nhi - lc.g0) * sd;
    lc.tau_c = bounded ? (zlo + zhi) : 0.0;
    double emax = 0.0;
    bool exact = true;
    for (int j = 0; j < lc.G; ++j) {
        const double D = ((double)lc.grid[j] - (double)lc.grid[0]) * sd;
        lc.Dl[j] = D;
        lc.e[j] = D - (double)j * lc.delta;
        lc.h2[j] = 0.5 * lc.e[j] * lc.e[j];   // (kan_pp.hip's moment transforms read it; same order, same bits)
        const long double DL = D;
        lc.K[j] = (double)(std::exp(-DL * DL) * std::exp((long double)lc.tau_c * (long double)lc.e[j]));
        emax = std::max(emax, std::fabs(lc.e[j]));
        if (lc.e[j] != 0.0) exact = false;
    }
    // recurrence admissibility: bounded normalizer, no overflow of exp(-z0²) or
    // R^(G-1), and a centred 2nd-order correction accurate to < 1 ulp.
    lc.path = kan::PATH_DIRECT;
    if (lc.basis == KANODE_BASIS_RBF && bounded) {
        const double zmax = std::max(std::fabs(zlo), std::fabs(zhi));
        const double lim = (dtype == KANODE_F64) ? 600.0 : 80.0;
        const double tmax = (zhi - zlo) * emax;   // max |τ' e_j|
        const bool ok = zmax * zmax <= lim && 2.0 * zmax * std::fabs(lc.delta) * (lc.G - 1) <= lim &&
                        lc.delta > 0.0 && (dtype == KANODE_F64 ? tmax <= 1e-5 : tmax <= 1e-3);
        if (ok) lc.path = exact ? kan::PATH_REC : kan::PATH_REC_CORR;
    }
    return KANODE_OK;
}

// Piecewise-polynomial table constants for a pointwise KDense(1,1,G) (kan_pp.hip).
// Interval width: the largest power of two <= 0.16·h_u, h_u the knot spacing seen
// in u (h / max N'(u)), capped at 1/16; with degree 9 the Chebyshev interpolation
// error of a Gaussian of width h_u is then <= ~1e-16 of |C|.  ni <= 512 intervals
// centred on 0 (so softsign's kink at 0 is an interval edge).
void make_pp_const(const LayerConst& lc, int dtype, int64_t nx, kan::PPConst& pc) {
    std::memset(&pc, 0, sizeof(pc));
    pc.enabled = dtype == KANODE_F64 && (lc.basis == KANODE_BASIS_RBF || lc.basis == KANODE_BASIS_RSWAF) &&
                 nx >= 2 && nx % 2 == 0;
    const double slope = (lc.norm == KANODE_NORM_SIGMOID || lc.norm == KANODE_NORM_SIGMOID_FAST) ? 0.25 : 1.0;
    const double hu = (1.0 / (double)lc.invh) / slope;
    double w = 1.0 / 16.0;
    while (w > 0.16 * hu && w > 0x1p-20) w *= 0.5;
    int ni = kan::kPPMaxIntervals;
    while (ni > 16 && ni * w > 8.0) ni >>= 1;   // domain at most [-4, 4)
    pc.ni = ni;
    pc.w = w;
    pc.inv_w = 1.0 / w;
    pc.x0 = ni / 2;
    pc.lo = -(ni / 2) * w;
    pc.tol = 2e-14;
    const int N = kan::kPPCoef;
    const long double pi = 3.141592653589793238462643383279502884L;
    for (int m = 0; m < N; ++m) pc.xi[m] = (double)std::cos(pi * (2 * m + 1) / (2.0L * N));
    pc.tchk[0] = -1.0;
    pc.tchk[1] = 0.0;
    pc.tchk[2] = 1.0;
    // Q = (Chebyshev -> monomial) · DCT, in long double
    long double T[kan::kPPCoef][kan::kPPCoef] = {};
    T[0][0] = 1;
    T[1][1] = 1;
    for (int l = 2; l < N; ++l) {
        for (int i = 1; i < N; ++i) T[l][i] = 2 * T[l - 1][i - 1];
        for (int i = 0; i < N; ++i) T[l][i] -= T[l - 2][i];
    }
    for (int i = 0; i < N; ++i)
        for (int m = 0; m < N; ++m) {
            long double s = 0;
            for (int l = 0; l < N; ++l) {
                const long double d = (2.0L / N) * std::cos(pi * l * (2 * m + 1) / (2.0L * N)) * (l == 0 ? 0.5L : 1.0L);
                s += T[l][i] * d;
            }
            pc.Q[i][m] = (double)s;
        }
}

int64_t layer_P(const LayerConst& lc) {
    return (int64_t)lc.O * lc.G * lc.I + (lc.use_base ? (int64_t)lc.O * lc.I : 0);
}

kanode_status stage_alloc(kanode_handle* h, size_t bytes) {
    HIP_TRY(h, h->stage.reserve(bytes));
    return KANODE_OK;
}

}  // namespace

extern "C" {

int32_t kanode_abi_version(void) { return KANODE_ABI_VERSION; }

const char* kanode_status_string(kanode_status s) {
    switch (s) {
    case KANODE_OK: return "ok";
    case KANODE_ERR_INVALID_ARG: return "invalid argument";
    case KANODE_ERR_UNSUPPORTED: return "unsupported configuration";
    case KANODE_ERR_HIP: return "HIP runtime error";
    case KANODE_ERR_ALLOC: return "allocation failure";
    case KANODE_ERR_CAPTURE: return "allocation needed during stream capture";
    }
    return "unknown status";
}

const char* kanode_last_error(const kanode_handle* h) { return h ? h->err.c_str() : "null handle"; }

kanode_status kanode_create(const kanode_spec* spec, kanode_handle** out) {
    if (!spec || !out) return KANODE_ERR_INVALID_ARG;
    *out = nullptr;
    kanode_handle* h = new (std::nothrow) kanode_handle();
    if (!h) return KANODE_ERR_ALLOC;
    h->spec = *spec;
    auto bail = [&](kanode_status s) {
        // keep the handle so the caller can read kanode_last_error, then destroy
        *out = h;
        return s;
    };
    if (spec->dtype != KANODE_F32 && spec->dtype != KANODE_F64)
        return bail(fail(h, KANODE_ERR_INVALID_ARG, "dtype must be KANODE_F32 or KANODE_F64"));
    h->esize = spec->dtype == KANODE_F64 ? 8 : 4;
    if (spec->n_layers < 1 || spec->n_layers > KANODE_MAX_LAYERS)
        return bail(fail(h, KANODE_ERR_INVALID_ARG, "n_layers must be in [1, 8]"));
    h->n_layers = spec->n_layers;
    int64_t off = 0;
    for (int l = 0; l < h->n_layers; ++l) {
        kanode_status s = make_layer_const(h, spec->layers[l], spec->dtype, off, h->hlc[l]);
        if (s != KANODE_OK) return bail(s);
        if (l > 0 && spec->layers[l].in_dims != spec->layers[l - 1].out_dims)
            return bail(fail(h, KANODE_ERR_INVALID_ARG,
                             "layer " + std::to_string(l) + " in_dims != previous out_dims (Lux.Chain)"));
        off += layer_P(h->hlc[l]);
        h->max_layer_P = std::max<int>(h->max_layer_P, (int)layer_P(h->hlc[l]));
        h->max_dim = std::max({h->max_dim, h->hlc[l].I, h->hlc[l].O});
        // kernel class for this layer
        const LayerConst& lc = h->hlc[l];
        const size_t rows = (size_t)(lc.G * lc.I + lc.I);
        if (lc.O <= 16 && (size_t)(lc.G * lc.I + lc.O + lc.I) * 65 * h->esize <= 150 * 1024 &&
            layer_P(lc) <= 64 * 32) {
            h->kind[l] = KIND_COL;
        } else if (lc.O <= kan::kWideOMax) {
            h->kind[l] = KIND_WIDE_IN;
        } else if (rows * kan::kWideKT * h->esize <= 150 * 1024) {
            h->kind[l] = KIND_WIDE_OUT;
        } else {
            return bail(fail(h, KANODE_ERR_UNSUPPORTED,
                             "layer " + std::to_string(l) + " shape (I=" + std::to_string(lc.I) + ", O=" +
                                 std::to_string(lc.O) + ") is not supported by this build"));
        }
    }
    h->P = off;
    if (spec->rhs_kind == KANODE_RHS_CHAIN) {
        h->n_in = spec->layers[0].in_dims;
        h->n_out = spec->layers[h->n_layers - 1].out_dims;
    } else if (spec->rhs_kind == KANODE_RHS_POINTWISE_PERIODIC_LAPLACIAN) {
        if (h->n_layers != 1 || spec->layers[0].in_dims != 1 || spec->layers[0].out_dims != 1)
            return bail(fail(h, KANODE_ERR_INVALID_ARG, "pointwise RHS needs exactly one KDense(1, 1, G)"));
        if (spec->nx < 1 || spec->nx > (1 << 30)) return bail(fail(h, KANODE_ERR_INVALID_ARG, "nx must be >= 1"));
        if (!(spec->dx > 0.0)) return bail(fail(h, KANODE_ERR_INVALID_ARG, "dx must be > 0"));
        h->n_in = h->n_out = spec->nx;
    } else {
        return bail(fail(h, KANODE_ERR_INVALID_ARG, "unknown rhs_kind"));
    }
    hipError_t e = hipSetDevice(spec->device);
    if (e != hipSuccess) return bail(fail(h, KANODE_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e)));
    if ((e = h->dlc_buf.reserve(sizeof(LayerConst) * h->n_layers)) != hipSuccess)
        return bail(fail(h, KANODE_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e)));
    if ((e = hipMemcpy(h->dlc(), h->hlc, sizeof(LayerConst) * h->n_layers, hipMemcpyHostToDevice)) != hipSuccess)
        return bail(fail(h, KANODE_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e)));
    if (spec->rhs_kind == KANODE_RHS_POINTWISE_PERIODIC_LAPLACIAN) {
        make_pp_const(h->hlc[0], spec->dtype, spec->nx, h->hpc);
        if (h->hpc.enabled) {
            if ((e = h->dpc_buf.reserve(sizeof(kan::PPConst))) != hipSuccess ||
                (e = hipMemcpy(h->dpc(), &h->hpc, sizeof(kan::PPConst), hipMemcpyHostToDevice)) != hipSuccess ||
                (e = h->dtable_buf.reserve(sizeof(double) * kan::pp_tables_doubles(h->hpc.ni))) != hipSuccess ||
                (e = hipMemset(h->dtable(), 0, sizeof(double) * kan::pp_tables_doubles(h->hpc.ni))) != hipSuccess)
                return bail(fail(h, KANODE_ERR_HIP, std::string("pp table: ") + hipGetErrorString(e)));
            h->opt.pp_on = 1;
            if (kan::fk_vjp_pp_supported(h->hlc[0], (int)spec->nx)) {
                kanode_status s = ensure_adjoint_slabs(h, nullptr, true);
                if (s != KANODE_OK) return bail(s);
            }
        }
    }
    // per-block partial rows: the column-kernel VJPs need a layer's (an all-column chain's) P per row;
    // the wide kernels keep their partials in the chain workspace; stage / error / table-VJP rows
    // need at most kMaxGrid + 2 doubles
    int64_t col_P = 0;
    for (int l = 0; l < h->n_layers; ++l)
        if (h->kind[l] == KIND_COL) col_P = std::max<int64_t>(col_P, layer_P(h->hlc[l]));
    if (all_col(h)) col_P = std::max<int64_t>(col_P, h->P);
    const size_t row = std::max<size_t>((size_t)col_P * h->esize, (size_t)(kan::kMaxGrid + 2) * sizeof(double));
    if ((e = h->slab.reserve((size_t)kSlabBlocks * row)) != hipSuccess)
        return bail(fail(h, KANODE_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e)));
    *out = h;
    return KANODE_OK;
}

void kanode_destroy(kanode_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->spec.device);
    if (h->solve_cache) kanode_solution_free(h->solve_cache);
    delete h;   // (its buffers free themselves)
}

int64_t kanode_param_length(const kanode_handle* h) { return h ? h->P : -1; }
int64_t kanode_layer_param_length(const kanode_handle* h, int32_t layer) {
    if (!h || layer < 0 || layer >= h->n_layers) return -1;
    return layer_P(h->hlc[layer]);
}
int64_t kanode_state_length(const kanode_handle* h) { return h ? h->n_in : -1; }

kanode_status kanode_knots(const kanode_handle* h, int32_t layer, float* grid_out) {
    if (!h || !grid_out || layer < 0 || layer >= h->n_layers) return KANODE_ERR_INVALID_ARG;
    std::memcpy(grid_out, h->hlc[layer].grid, sizeof(float) * h->hlc[layer].G);
    return KANODE_OK;
}

kanode_status kanode_reserve(kanode_handle* h, int64_t max_batch) {
    kanode_status s = check_handle(h);
    if (s != KANODE_OK) return s;
    if (max_batch < 0) return fail(h, KANODE_ERR_INVALID_ARG, "max_batch < 0");
    s = ensure_ws(h, max_batch, nullptr);
    if (s != KANODE_OK) return s;
    if (h->spec.rhs_kind == KANODE_RHS_POINTWISE_PERIODIC_LAPLACIAN) {
        if ((size_t)(h->spec.nx * max_batch) * h->esize > h->ws.bytes()) HIP_TRY(h, hipDeviceSynchronize());   // (every stream)
        if ((s = ensure_fk_ws(h, max_batch, nullptr)) != KANODE_OK) return s;
    }
    // Reset the table stamps: re-zeroing the stamp region here (the call before graph capture / a
    // new batch) invalidates every build block's stamp, so the next launch rebuilds every table.
    if (h->dtable()) {
        const int64_t off = (int64_t)kan::kPPMaxFns * kan::kPPCoef * h->hpc.ni;
        HIP_TRY(h, hipDeviceSynchronize());
        HIP_TRY(h, hipMemset(h->dtable() + off, 0, sizeof(double) * (size_t)(kan::pp_tables_doubles(h->hpc.ni) - off)));
    }
    h->reserved_batch = std::max(h->reserved_batch, max_batch);
    return KANODE_OK;
}

kanode_status kanode_set_option(kanode_handle* h, int32_t option, int64_t value) {
    if (!h) return KANODE_ERR_INVALID_ARG;
    std::string msg;   // (filled only by a refusal)
    const kanode_status s = options_set(h->opt, option, value, h->hpc.enabled != 0, msg);
    return s == KANODE_OK ? s : fail(h, s, msg);
}

int64_t kanode_get_option(const kanode_handle* h, int32_t option) { return h ? options_get(h->opt, option) : -1; }

kanode_status kanode_set_l1_penalty(kanode_handle* h, double act_reg) {
    if (!h) return KANODE_ERR_INVALID_ARG;
    if (!(act_reg >= 0.0) || !std::isfinite(act_reg))
        return fail(h, KANODE_ERR_INVALID_ARG, "kanode_set_l1_penalty: act_reg must be finite and >= 0");
    h->l1_penalty = act_reg;
    return KANODE_OK;
}

double kanode_get_l1_penalty(const kanode_handle* h) { return h ? h->l1_penalty : 0.0; }

kanode_status kanode_rhs_host(kanode_handle* h, const void* p, const void* u, void* du, int64_t batch) {
    kanode_status s = check_handle(h);
    if (s != KANODE_OK) return s;
    if (batch <= 0) return batch == 0 ? KANODE_OK : fail(h, KANODE_ERR_INVALID_ARG, "batch < 0");
    const size_t bp = (size_t)h->P * h->esize, bu = (size_t)(h->n_in * batch) * h->esize,
                 bo = (size_t)(h->n_out * batch) * h->esize;
    if ((s = stage_alloc(h, bp + bu + bo)) != KANODE_OK) return s;
    char* d = (char*)h->stage.ptr();
    HIP_TRY(h, hipMemcpy(d, p, bp, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(d + bp, u, bu, hipMemcpyHostToDevice));
    if ((s = kanode_rhs(h, d, d + bp, d + bp + bu, batch, nullptr)) != KANODE_OK) return s;
    HIP_TRY(h, hipMemcpy(du, d + bp + bu, bo, hipMemcpyDeviceToHost));
    return KANODE_OK;
}

kanode_status kanode_vjp_host(kanode_handle* h, const void* p, const void* u, const void* lam, void* lam_J, void* dp,
                              int64_t batch) {
    kanode_status s = check_handle(h);
    if (s != KANODE_OK) return s;
    if (batch <= 0) return batch == 0 ? KANODE_OK : fail(h, KANODE_ERR_INVALID_ARG, "batch < 0");
    const size_t bp = (size_t)h->P * h->esize, bu = (size_t)(h->n_in * batch) * h->esize,
                 bo = (size_t)(h->n_out * batch) * h->esize;
    if ((s = stage_alloc(h, 2 * bp + 2 * bu + bo)) != KANODE_OK) return s;
    char* d = (char*)h->stage.ptr();
    char* dp_d = d + bp;
    char* u_d = dp_d + bp;
    char* lam_d = u_d + bu;
    char* lj_d = lam_d + bo;
    HIP_TRY(h, hipMemcpy(d, p, bp, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(u_d, u, bu, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(lam_d, lam, bo, hipMemcpyHostToDevice));
    if (dp) HIP_TRY(h, hipMemcpy(dp_d, dp, bp, hipMemcpyHostToDevice));
    if ((s = kanode_vjp(h, d, u_d, lam_d, lam_J ? lj_d : nullptr, dp ? dp_d : nullptr, batch, nullptr)) != KANODE_OK)
        return s;
    if (lam_J) HIP_TRY(h, hipMemcpy(lam_J, lj_d, bu, hipMemcpyDeviceToHost));
    if (dp) HIP_TRY(h, hipMemcpy(dp, dp_d, bp, hipMemcpyDeviceToHost));
    return KANODE_OK;
}

kanode_status kanode_adam_step(void* x, void* m, void* v, const void* g, int64_t n, int32_t dtype, double scale,
                               double eta, double beta1, double beta2, double eps, double beta1_t, double beta2_t,
                               void* stream) {
    if (n < 0 || (dtype != KANODE_F32 && dtype != KANODE_F64)) return KANODE_ERR_INVALID_ARG;
    if (n == 0) return KANODE_OK;
    if (!x || !m || !v || !g) return KANODE_ERR_INVALID_ARG;
    // 1 - β^t must stay positive (t >= 1 with 0 <= β < 1): the bias corrections divide by it
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && beta1_t < 1.0 && beta2_t < 1.0))
        return KANODE_ERR_INVALID_ARG;
    kan::AdamArgs a;
    a.scale = scale;
    a.beta1 = beta1;
    a.beta2 = beta2;
    a.omb1 = 1.0 - beta1;
    a.omb2 = 1.0 - beta2;
    a.c1 = 1.0 - beta1_t;
    a.c2 = 1.0 - beta2_t;
    a.eps = eps;
    a.eta = eta;
    const hipStream_t st = (hipStream_t)stream;
    const hipError_t e = by_dtype((int)dtype, [&](auto t) {
        using T = decltype(t);
        return kan::launch_adam_step<T>((T*)x, (T*)m, (T*)v, (const T*)g, n, a, st);
    });
    return e == hipSuccess ? KANODE_OK : KANODE_ERR_HIP;
}

kanode_status kanode_table_rejections(kanode_handle* h, int32_t out[3]) {
    if (!h || !out) return KANODE_ERR_INVALID_ARG;
    if (!h->dtable() || !h->opt.pp_on) return fail(h, KANODE_ERR_UNSUPPORTED, "no pointwise table on this handle");
    const int ni = h->hpc.ni, nb = ni / kan::kPPPerBlock;
    const int64_t off = (int64_t)kan::kPPMaxFns * kan::kPPCoef * ni;
    std::vector<double> st((size_t)kan::kPPMaxFns * nb * kan::kPPStampStride);
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(st.data(), h->dtable() + off, st.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int f = 0; f < kan::kPPMaxFns; ++f) {
        int32_t n = 0;
        bool built = true;
        for (int b = 0; b < nb; ++b) {
            const double* sp = st.data() + ((size_t)f * nb + b) * kan::kPPStampStride;
            if (sp[kan::kPPStampValid] != 1.0) built = false;
            else n += (int32_t)sp[kan::kPPStampRejected];
        }
        out[f] = built ? n : -1;
    }
    return KANODE_OK;
}

kanode_status kanode_last_fk_launch(kanode_handle* h, int32_t out[8]) {
    if (!h || !out) return KANODE_ERR_INVALID_ARG;
    const kan::FkLaunchRec& r = h->fk_launch;
    out[0] = r.family;
    out[1] = r.np;
    out[2] = r.norm;
    out[3] = r.path;
    out[4] = r.gt;
    out[5] = (r.ni_ct == 256 ? 1 : 0) | (r.combine << 1) | (r.fused_finish << 3);
    out[6] = r.chunk;
    out[7] = r.grid;
    return KANODE_OK;
}

int64_t kanode_adjoint_step_sizes(const kanode_handle* h, double* out, int64_t cap) {
    if (!h) return -1;
    const int64_t n = (int64_t)h->adj_steps.size();
    if (out && cap > 0) std::memcpy(out, h->adj_steps.data(), (size_t)std::min(n, cap) * sizeof(double));
    return n;
}

}  // extern "C"

// ---- the integrator's accessors (kanode_internal.hpp) ----
kanode_status kanode_internal_fail(kanode_handle* h, kanode_status s, const std::string& msg) { return fail(h, s, msg); }
kanode_status kanode_internal_check(kanode_handle* h) { return check_handle(h); }
int kanode_internal_dtype(const kanode_handle* h) { return h->spec.dtype; }
int64_t kanode_internal_state_length(const kanode_handle* h) { return h->n_in; }
int64_t kanode_internal_param_length(const kanode_handle* h) { return h->P; }
bool kanode_internal_square(const kanode_handle* h) { return h->n_in == h->n_out; }
void kanode_internal_hold_tables(kanode_handle* h, bool on) {
    h->hold_tables = on;
    h->built_phi = h->built_vjp = false;
}
double* kanode_internal_scratch(kanode_handle* h) { return (double*)h->slab.ptr(); }
int kanode_internal_scratch_rows(const kanode_handle*) { return kSlabBlocks; }
int kanode_internal_max_parts() { return kSlabBlocks; }
void kanode_internal_set_err_parts(kanode_handle* h, double* parts, int* nparts) {
    h->err_parts = parts;
    h->err_nparts = nparts;
}
void* kanode_internal_solution_cache(kanode_handle* h) { return &h->solve_cache; }
int kanode_internal_fused_solve_cap(const kanode_handle* h) { return h->opt.fused_solve_cap; }
void kanode_internal_set_last_adjoint(kanode_handle* h, int path) { h->opt.last_adjoint = path; }
void kanode_internal_clear_adjoint_steps(kanode_handle* h) { h->adj_steps.clear(); }
std::vector<double>* kanode_internal_adjoint_steps(kanode_handle* h) {
    return h->opt.record_adj_steps ? &h->adj_steps : nullptr;
}
