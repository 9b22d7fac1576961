# KANODEHip.jl — Julia binding of libkanode.so (include/kanode.h), the shim a maintainer adds next to
# src/KolmogorovArnold.jl of the reference (INTEGRATION.md).  Not compiled or executed here: Julia is
# absent from this image.  tests/test_julia_shim.py checks it textually against the C header (every
# ccall'd symbol is declared, every mirrored struct has the header's fields in order) and checks that
# the Lux / ChainRules surface below exists and that every kernel call is guarded by the shape checks.
#
# What it replaces (file:line relative to the reference):
#   KANChainHip      Lux.Chain(KDense(...), KDense(...))           Lotka-Volterra/LV_driver_KANODE.jl:139-143
#                    incl. Lux.setup / ComponentArray(pM) axes      :143,162,173-175 (kdense.jl:70-107)
#   RCKanodeHip      rc_kanode(u, p, t)                             PDE examples/Fisher-KPP_Source.jl:95-98
#   solve_tsit5      solve(ODEProblem(f, u0, tspan, p), Tsit5(); saveat) + its InterpolatingAdjoint
#                                                                   LV_driver_KANODE.jl:180-184,
#                                                                   Fisher-KPP_Source.jl:102-103,198
module KANODEHip

using LuxCore, ChainRulesCore, Libdl, Random
using WeightInitializers: glorot_uniform

const LIB = Ref{Ptr{Cvoid}}(C_NULL)
function lib()
    if LIB[] == C_NULL
        LIB[] = Libdl.dlopen(get(ENV, "KANODE_LIB", "libkanode.so"))
    end
    return LIB[]
end
sym(s::Symbol) = Libdl.dlsym(lib(), s)
const HIPLIB = "libamdhip64"

# ---- mirrors of the C structs (include/kanode.h) ------------------------------------------------
# mirrors kanode_layer_spec
struct LayerSpec
    in_dims::Int32; out_dims::Int32; grid_len::Int32
    normalizer::Int32; basis::Int32; use_base_act::Int32
    grid_lo::Float32; grid_hi::Float32; denominator::Float32
    iqf_reference_quirk::Int32
end
# mirrors kanode_spec
struct Spec
    n_layers::Int32
    layers::NTuple{8,LayerSpec}
    dtype::Int32; rhs_kind::Int32
    nx::Int64; diffusion::Float64; dx::Float64
    device::Int32
end

const NORM = Dict(:tanh_fast => 0, :tanh => 1, :softsign => 2, :sigmoid => 3, :σ => 3, :sigmoid_fast => 4,
                  :identity => 5)
const BASIS = Dict(:rbf => 0, :rswaf => 1, :iqf => 2)
# NNlib.fast_act under allow_fast_activation = true (kdense.jl:57-61): tanh -> tanh_fast, sigmoid -> sigmoid_fast
const FAST = Dict(:tanh => :tanh_fast, :sigmoid => :sigmoid_fast, :σ => :sigmoid_fast)
const DTYPE = Dict(Float32 => Int32(0), Float64 => Int32(1))

# the drivers pass the functions themselves (basis_func = rbf, normalizer = softsign); Symbols work too
actname(f::Symbol) = f
actname(f::Function) = nameof(f)

"""layerspec(in, out, G; normalizer, basis_func, use_base_act, grid_lims, denominator, ...) — the KDense
constructor arguments (kdense.jl:20-37), with the reference's defaults: normalizer = tanh (fast_act ->
tanh_fast), basis_func = rbf, use_base_act = true, grid_lims = (-1f0, 1f0), denominator = Float32(2/(G-1))."""
function layerspec(I::Integer, O::Integer, G::Integer; normalizer = :tanh, basis_func = :rbf,
                   use_base_act::Bool = true, grid_lims = (-1.0f0, 1.0f0), denominator = Float32(2 / (G - 1)),
                   allow_fast_activation::Bool = true, iqf_reference_quirk::Bool = true)
    n = actname(normalizer)
    if allow_fast_activation
        n = get(FAST, n, n)
    end
    haskey(NORM, n) || throw(ArgumentError("normalizer $n is not implemented by libkanode"))
    b = actname(basis_func)
    haskey(BASIS, b) || throw(ArgumentError("basis_func $b is not implemented by libkanode"))
    return LayerSpec(Int32(I), Int32(O), Int32(G), Int32(NORM[n]), Int32(BASIS[b]), Int32(use_base_act),
                     Float32(grid_lims[1]), Float32(grid_lims[2]), Float32(denominator), Int32(iqf_reference_quirk))
end
pad(ls) = ntuple(i -> i <= length(ls) ? ls[i] : layerspec(1, 1, 2), 8)

# ---- the handle ----------------------------------------------------------------------------------
mutable struct Handle
    ptr::Ptr{Cvoid}
    T::DataType        # element type of u, p and every output (Float32 or Float64)
    P::Int             # kanode_param_length: the flat ComponentArray length
    nin::Int           # rows of the [N, B] input
    nout::Int          # rows of the [N, B] output
end
errmsg(ptr::Ptr{Cvoid}) = unsafe_string(ccall(sym(:kanode_last_error), Cstring, (Ptr{Cvoid},), ptr))
function Handle(ls::Vector{LayerSpec}; T::Type = Float64, rhs_kind::Integer = 0, nx::Integer = 0, D::Real = 0.0,
                dx::Real = 1.0, device::Integer = 0)
    haskey(DTYPE, T) || throw(ArgumentError("libkanode computes in Float32 or Float64, not $T"))
    s = Ref(Spec(Int32(length(ls)), pad(ls), DTYPE[T], Int32(rhs_kind), Int64(nx), Float64(D), Float64(dx),
                 Int32(device)))
    out = Ref{Ptr{Cvoid}}(C_NULL)
    st = ccall(sym(:kanode_create), Cint, (Ref{Spec}, Ref{Ptr{Cvoid}}), s, out)
    if st != 0
        msg = out[] == C_NULL ? unsafe_string(ccall(sym(:kanode_status_string), Cstring, (Cint,), st)) :
              errmsg(out[])
        out[] == C_NULL || ccall(sym(:kanode_destroy), Cvoid, (Ptr{Cvoid},), out[])
        error("kanode_create: ", msg)
    end
    P = Int(ccall(sym(:kanode_param_length), Int64, (Ptr{Cvoid},), out[]))
    nin = rhs_kind == 1 ? Int(nx) : Int(ls[1].in_dims)
    nout = rhs_kind == 1 ? Int(nx) : Int(ls[end].out_dims)
    h = Handle(out[], T, P, nin, nout)
    finalizer(x -> ccall(sym(:kanode_destroy), Cvoid, (Ptr{Cvoid},), x.ptr), h)
    return h
end
check(h::Handle, st) = st == 0 || error("libkanode: ", errmsg(h.ptr))

# Host copies in the handle's element type.  Duals (ForwardDiff) cannot go through the kernels: the
# automatic sensealg of a small problem (ForwardDiffSensitivity, e.g. Fisher-KPP at Nx = 26) must be
# replaced by InterpolatingAdjoint(autojacvec = ZygoteVJP()), whose VJPs are the rrules below.
function tohost(::Type{T}, a::AbstractArray) where {T}
    eltype(a) <: Real && !(eltype(a) <: Bool) ||
        throw(ArgumentError("libkanode takes real arrays, got eltype $(eltype(a))"))
    eltype(a) <: Union{Float32,Float64,Integer} ||
        throw(ArgumentError("eltype $(eltype(a)) cannot enter the HIP kernels (forward-mode AD?): solve with " *
                            "sensealg = InterpolatingAdjoint(autojacvec = ZygoteVJP())"))
    return a isa Array{T} ? a : Array{T}(a)
end

# every kernel call goes through these checks: the C side trusts the sizes it is given
function checkp(h::Handle, p::AbstractVector)
    length(p) == h.P || throw(DimensionMismatch("p has length $(length(p)); the KAN has $(h.P) parameters " *
                                                "(kanode_param_length)"))
    return nothing
end
function checku(h::Handle, u::AbstractVecOrMat, rows::Int, what::String)
    size(u, 1) == rows || throw(DimensionMismatch("$what has $(size(u, 1)) rows; the handle expects $rows"))
    return nothing
end

"""rhs(h, p, u) -> du: kanode_rhs_host on a Julia [N] or [N, B] array."""
function rhs(h::Handle, p::AbstractVector, u::AbstractVecOrMat)
    checkp(h, p)
    checku(h, u, h.nin, "u")
    T = h.T
    pv, uc = tohost(T, p), tohost(T, u)
    B = size(uc, 2)
    du = Matrix{T}(undef, h.nout, B)
    GC.@preserve pv uc du check(h, ccall(sym(:kanode_rhs_host), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64), h.ptr, pv, uc, du, B))
    return u isa AbstractVector ? vec(du) : du
end

"""vjp(h, p, u, λ) -> (λᵀ∂f/∂u, λᵀ∂f/∂p): kanode_vjp_host (dp starts at zero)."""
function vjp(h::Handle, p::AbstractVector, u::AbstractVecOrMat, λ::AbstractVecOrMat)
    checkp(h, p)
    checku(h, u, h.nin, "u")
    checku(h, λ, h.nout, "λ")
    size(λ, 2) == size(u, 2) || throw(DimensionMismatch("λ and u have different batch sizes"))
    h.nin == h.nout || throw(ArgumentError("the RHS VJP needs a chain with in_dims == out_dims"))
    T = h.T
    pv, uc, λc = tohost(T, p), tohost(T, u), tohost(T, λ)
    B = size(uc, 2)
    λJ = similar(uc)
    dp = zeros(T, h.P)
    GC.@preserve pv uc λc λJ dp check(h, ccall(sym(:kanode_vjp_host), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64),
        h.ptr, pv, uc, λc, λJ, dp, B))
    return λJ, dp
end

# p̄ in p's own type: a ComponentArray keeps its axes (similar), a Vector stays a Vector
ptangent(p::Vector, dp) = dp
ptangent(p::AbstractVector, dp) = copyto!(similar(p, eltype(dp)), dp)
xtangent(x::AbstractVector, g) = vec(g)
xtangent(x::AbstractMatrix, g) = g

# ---- the Lux layer -------------------------------------------------------------------------------
"""KANChainHip(layerspecs; T) — a whole KDense chain as one Lux layer, the drop-in for
`Lux.Chain(KDense(...), KDense(...))` inside NeuralODE (LV_driver_KANODE.jl:139-143,180).
`Lux.setup(rng, kan1)` returns the reference's (layer_1 = (C, W), layer_2 = (C, W)) parameters with the
same Glorot-uniform Float32 init and RNG order (kdense.jl:70-86), so `ComponentArray(pM)` has the
reference axes and `getdata(ComponentArray(pM)) ./ 1e5` (:173-175) is the flat vector the kernels take."""
struct KANChainHip <: LuxCore.AbstractLuxLayer
    h::Handle
    specs::Vector{LayerSpec}
end
KANChainHip(ls::Vector{LayerSpec}; T::Type = Float64, device::Integer = 0) = KANChainHip(Handle(ls; T, device), ls)

layernames(l::KANChainHip) = ntuple(i -> Symbol("layer_", i), length(l.specs))

function initlayer(rng::AbstractRNG, s::LayerSpec)
    C = glorot_uniform(rng, Int(s.out_dims), Int(s.grid_len) * Int(s.in_dims))   # [O, G·I]  kdense.jl:74
    if s.use_base_act == 1
        return (; C, W = glorot_uniform(rng, Int(s.out_dims), Int(s.in_dims)))   # kdense.jl:80
    end
    return (; C)
end
function LuxCore.initialparameters(rng::AbstractRNG, l::KANChainHip)
    return NamedTuple{layernames(l)}(ntuple(i -> initlayer(rng, l.specs[i]), length(l.specs)))
end
# st = (grid = collect(LinRange(grid_lims..., G)),) per layer (kdense.jl:88-92)
function LuxCore.initialstates(::AbstractRNG, l::KANChainHip)
    g(s) = (; grid = collect(LinRange(s.grid_lo, s.grid_hi, Int(s.grid_len))))
    return NamedTuple{layernames(l)}(ntuple(i -> g(l.specs[i]), length(l.specs)))
end
LuxCore.parameterlength(l::KANChainHip) = l.h.P
LuxCore.statelength(l::KANChainHip) = sum(Int(s.grid_len) for s in l.specs)

# the flat parameter vector in ComponentArray order (layer_1.C, layer_1.W, layer_2.C, ...)
flatp(p::AbstractVector) = p
flatp(p::NamedTuple) = reduce(vcat, [vec(q) for layer in values(p) for q in values(layer)])

(l::KANChainHip)(x::AbstractVecOrMat, p, st) = (rhs(l.h, flatp(p), x), st)

function ChainRulesCore.rrule(l::KANChainHip, x::AbstractVecOrMat, p::AbstractVector, st)
    y = rhs(l.h, p, x)
    function kanchain_pullback(Δ)
        ȳ = unthunk(unthunk(Δ)[1])
        if ȳ isa AbstractZero
            return (NoTangent(), ZeroTangent(), ZeroTangent(), NoTangent())
        end
        λJ, dp = vjp(l.h, p, x, ȳ)
        return (NoTangent(), xtangent(x, λJ), ptangent(p, dp), NoTangent())
    end
    return (y, st), kanchain_pullback
end

# ---- Fisher-KPP: replaces rc_kanode (PDE examples/Fisher-KPP_Source.jl:95-98) ----------------------
fk_handle(nx::Integer, dx::Real; D::Real = 0.01, G::Integer = 10, normalizer = :softsign, basis_func = :rbf,
          T::Type = Float64, device::Integer = 0) =
    Handle([layerspec(1, 1, G; normalizer, basis_func)]; T, rhs_kind = 1, nx, D, dx, device)

"""rc_kanode_hip(h)(u, p, t) = D*lap*u + kan1_.(u), differentiable (rrule -> kanode_vjp_host)."""
struct RCKanodeHip
    h::Handle
end
rc_kanode_hip(h::Handle) = RCKanodeHip(h)
(f::RCKanodeHip)(u::AbstractVecOrMat, p::AbstractVector, t) = rhs(f.h, p, u)

function ChainRulesCore.rrule(f::RCKanodeHip, u::AbstractVecOrMat, p::AbstractVector, t)
    du = rhs(f.h, p, u)
    function rc_kanode_pullback(Δ)
        ḡ = unthunk(Δ)
        if ḡ isa AbstractZero
            return (NoTangent(), ZeroTangent(), ZeroTangent(), NoTangent())
        end
        λJ, dp = vjp(f.h, p, u, ḡ)
        return (NoTangent(), xtangent(u, λJ), ptangent(p, dp), NoTangent())
    end
    return du, rc_kanode_pullback
end

# ---- the whole solve + InterpolatingAdjoint on the device (kanode_solve_tsit5 / _adjoint_tsit5) -----
# mirrors kanode_solver_options
struct SolverOptions
    abstol::Float64; reltol::Float64; dt::Float64; adaptive::Int32
    maxiters::Int64; dtmin::Float64; beta1::Float64; beta2::Float64; gamma::Float64
    qmin::Float64; qmax::Float64; qoldinit::Float64
    control::Int32; graph_steps::Int32
end
function default_options()
    o = Ref{SolverOptions}()
    ccall(sym(:kanode_solver_options_default), Cvoid, (Ref{SolverOptions},), o)
    return o[]
end
"""options(; abstol = 1e-6, reltol = 1e-3, dt, adaptive, maxiters, control): solve()'s keywords, with the
OrdinaryDiffEq defaults (include/kanode.h kanode_solver_options)."""
function options(; abstol::Real = 1e-6, reltol::Real = 1e-3, dt::Real = 0.0, adaptive::Bool = true,
                 maxiters::Integer = 100000, control::Integer = 0)
    d = default_options()
    return SolverOptions(abstol, reltol, dt, Int32(adaptive), Int64(maxiters), d.dtmin, d.beta1, d.beta2, d.gamma,
                         d.qmin, d.qmax, d.qoldinit, Int32(control), d.graph_steps)
end
# mirrors kanode_solve_stats
struct SolveStats
    naccept::Int64; nreject::Int64; nf::Int64
end

# device buffers through the HIP runtime (no AMDGPU.jl: hipMalloc / hipMemcpy / hipFree only)
hipcheck(e, what) = e == 0 || error("$what failed with hipError $e")
mutable struct DevBuf
    ptr::Ptr{Cvoid}
    nbytes::Int
end
function DevBuf(nbytes::Integer)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    hipcheck(ccall((:hipMalloc, HIPLIB), Cint, (Ref{Ptr{Cvoid}}, Csize_t), r, max(nbytes, 1)), "hipMalloc")
    b = DevBuf(r[], Int(nbytes))
    finalizer(x -> ccall((:hipFree, HIPLIB), Cint, (Ptr{Cvoid},), x.ptr), b)
    return b
end
function upload(a::Array)
    b = DevBuf(sizeof(a))
    GC.@preserve a hipcheck(ccall((:hipMemcpy, HIPLIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Cint),
                                  b.ptr, a, sizeof(a), 1), "hipMemcpy H2D")
    return b
end
function download!(a::Array, b::DevBuf)
    sizeof(a) <= b.nbytes || throw(DimensionMismatch("device buffer smaller than the host array"))
    GC.@preserve a hipcheck(ccall((:hipMemcpy, HIPLIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Cint),
                                  a, b.ptr, sizeof(a), 2), "hipMemcpy D2H")
    return a
end

# the forward dense output (kanode_solution), freed with the object
mutable struct DenseOutput
    ptr::Ptr{Cvoid}
end
function DenseOutput(ptr::Ptr{Cvoid})
    d = DenseOutput(ptr)
    finalizer(x -> (x.ptr == C_NULL || ccall(sym(:kanode_solution_free), Cvoid, (Ptr{Cvoid},), x.ptr)), d)
    return d
end

# raw entry points on device pointers: returns (stats, dense::Ptr) ; dense feeds adjoint!, then free_dense
function solve!(h::Handle, p::Ptr{Cvoid}, u0::Ptr{Cvoid}, B::Integer, tspan, saveat::Vector{Float64},
                usave::Ptr{Cvoid}; opt::SolverOptions = default_options(), keep_dense::Bool = false,
                stream::Ptr{Cvoid} = C_NULL)
    st = Ref{SolveStats}()
    dense = Ref{Ptr{Cvoid}}(C_NULL)
    check(h, ccall(sym(:kanode_solve_tsit5), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Float64, Float64, Ptr{Float64}, Int64, Ptr{Cvoid},
         Ref{SolverOptions}, Ptr{Ptr{Cvoid}}, Ref{SolveStats}, Ptr{Cvoid}),
        h.ptr, p, u0, B, tspan[1], tspan[2], saveat, length(saveat), usave, opt,
        keep_dense ? dense : Ptr{Ptr{Cvoid}}(C_NULL), st, stream))
    return st[], dense[]
end
function adjoint!(h::Handle, p::Ptr{Cvoid}, dense::Ptr{Cvoid}, dl_du::Ptr{Cvoid}, du0::Ptr{Cvoid},
                  dp::Ptr{Cvoid}; opt::SolverOptions = default_options(), stream::Ptr{Cvoid} = C_NULL)
    st = Ref{SolveStats}()
    check(h, ccall(sym(:kanode_adjoint_tsit5), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{SolverOptions},
         Ref{SolveStats}, Ptr{Cvoid}), h.ptr, p, dense, dl_du, du0, dp, opt, st, stream))
    return st[]
end
free_dense(d::Ptr{Cvoid}) = ccall(sym(:kanode_solution_free), Cvoid, (Ptr{Cvoid},), d)

function solve_impl(h::Handle, u0::AbstractVecOrMat, tspan, p::AbstractVector, saveat::AbstractVector,
                    opt::SolverOptions, keep_dense::Bool)
    checkp(h, p)
    checku(h, u0, h.nin, "u0")
    h.nin == h.nout || throw(ArgumentError("an ODE RHS needs a chain with in_dims == out_dims"))
    T = h.T
    ts = Vector{Float64}(saveat)
    issorted(ts) || throw(ArgumentError("saveat must be ascending"))
    B = size(u0, 2)
    pd, ud = upload(tohost(T, p)), upload(tohost(T, u0))
    out = Array{T}(undef, h.nin, B, length(ts))
    od = DevBuf(sizeof(out))
    st, dense = solve!(h, pd.ptr, ud.ptr, B, tspan, ts, od.ptr; opt, keep_dense)
    download!(out, od)
    sol = u0 isa AbstractVector ? reshape(out, h.nin, length(ts)) : out
    return sol, st, (keep_dense ? DenseOutput(dense) : nothing), pd
end

"""solve_tsit5(h, u0, tspan, p, saveat; abstol, reltol, dt, adaptive) -> Array(sol): [N, n_save] for a
vector u0, [N, B, n_save] for a matrix (the layout of `Array(solve(prob, Tsit5(); saveat))`).
Differentiable in u0 and p by its rrule, whose pullback is kanode_adjoint_tsit5: SciMLSensitivity's
InterpolatingAdjoint, the NeuralODE default (LV_driver_KANODE.jl:180), on the device."""
function solve_tsit5(h::Handle, u0::AbstractVecOrMat, tspan, p::AbstractVector, saveat::AbstractVector; kw...)
    sol, _, _, _ = solve_impl(h, u0, tspan, p, saveat, options(; kw...), false)
    return sol
end

function ChainRulesCore.rrule(::typeof(solve_tsit5), h::Handle, u0::AbstractVecOrMat, tspan, p::AbstractVector,
                              saveat::AbstractVector; kw...)
    opt = options(; kw...)
    sol, _, dense, pd = solve_impl(h, u0, tspan, p, saveat, opt, true)
    function solve_tsit5_pullback(Δ)
        ū = unthunk(Δ)
        if ū isa AbstractZero
            return (NoTangent(), NoTangent(), ZeroTangent(), NoTangent(), ZeroTangent(), NoTangent())
        end
        T = h.T
        size(ū) == size(sol) || throw(DimensionMismatch("cotangent of the solution has the wrong shape"))
        gd = upload(tohost(T, ū))
        du0 = Array{T}(undef, size(u0))
        dp = Array{T}(undef, h.P)
        du0d, dpd = DevBuf(sizeof(du0)), DevBuf(sizeof(dp))
        adjoint!(h, pd.ptr, dense.ptr, gd.ptr, du0d.ptr, dpd.ptr; opt)
        download!(du0, du0d)
        download!(dp, dpd)
        return (NoTangent(), NoTangent(), du0, NoTangent(), ptangent(p, dp), NoTangent())
    end
    return sol, solve_tsit5_pullback
end

# --- ForwardDiffSensitivity (kanode_forward_sensitivity_tsit5): the gradient SciMLSensitivity 7.69 picks for the
# source-term drivers at their own sizes (Fisher-KPP_Source.jl:198, Zygote.gradient(loss, p) with no sensealg and
# length(u0) + length(p) <= 100): the Dual-number solve, one partial per parameter, on the device in one workgroup.
function fsens!(h::Handle, p::Ptr{Cvoid}, u0::Ptr{Cvoid}, B::Integer, tspan, saveat::Vector{Float64},
                usave::Ptr{Cvoid}, ssave::Ptr{Cvoid}; opt::SolverOptions = default_options(),
                stream::Ptr{Cvoid} = C_NULL)
    st = Ref{SolveStats}()
    check(h, ccall(sym(:kanode_forward_sensitivity_tsit5), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Float64, Float64, Ptr{Float64}, Int64, Ptr{Cvoid}, Ptr{Cvoid},
         Ref{SolverOptions}, Ref{SolveStats}, Ptr{Cvoid}),
        h.ptr, p, u0, B, tspan[1], tspan[2], saveat, length(saveat), usave, ssave, opt, st, stream))
    return st[]
end
fsens_supported(h::Handle, B::Integer) = ccall(sym(:kanode_forward_sensitivity_supported), Int32,
                                               (Ptr{Cvoid}, Int64), h.ptr, B) == 1
# KANODE_OPT_FSENS_WIDE (include/kanode.h): 1 = fields of 65 to 128 entries are covered too (two entries per lane)
const OPT_FSENS_WIDE = Int32(20)
fsens_wide!(h::Handle, v::Integer = 1) = check(h, ccall(sym(:kanode_set_option), Cint, (Ptr{Cvoid}, Int32, Int64),
                                                        h.ptr, OPT_FSENS_WIDE, v))

"""solve_tsit5_fwd(h, u0, tspan, p, saveat; abstol, reltol) -> Array(sol), like solve_tsit5, but differentiable in p
by forward sensitivities (ForwardDiffSensitivity, the reference's automatic choice for its small source-term
problems): the rrule's pullback contracts the cotangent with ∂u(saveat)/∂p, computed in the same solve."""
function solve_tsit5_fwd(h::Handle, u0::AbstractVecOrMat, tspan, p::AbstractVector, saveat::AbstractVector; kw...)
    sol, _ = fwd_impl(h, u0, tspan, p, saveat, options(; kw...))
    return sol
end
function fwd_impl(h::Handle, u0::AbstractVecOrMat, tspan, p::AbstractVector, saveat::AbstractVector,
                  opt::SolverOptions)
    checkp(h, p)
    checku(h, u0, h.nin, "u0")
    T = h.T
    ts = Vector{Float64}(saveat)
    issorted(ts) || throw(ArgumentError("saveat must be ascending"))
    B = size(u0, 2)
    fsens_supported(h, B) || fsens_wide!(h)     # (idempotent: the whole range SciMLSensitivity's rule selects)
    fsens_supported(h, B) || throw(ArgumentError("forward sensitivities: not covered for this handle / batch"))
    pd, ud = upload(tohost(T, p)), upload(tohost(T, u0))
    out = Array{T}(undef, h.nin, B, length(ts))
    S = Array{T}(undef, h.nin, B, h.P, length(ts))          # s_save [n_save, P, N, B] in column-major order
    od, sd = DevBuf(sizeof(out)), DevBuf(sizeof(S))
    fsens!(h, pd.ptr, ud.ptr, B, tspan, ts, od.ptr, sd.ptr; opt)
    download!(out, od)
    download!(S, sd)
    sol = u0 isa AbstractVector ? reshape(out, h.nin, length(ts)) : out
    return sol, S
end
function ChainRulesCore.rrule(::typeof(solve_tsit5_fwd), h::Handle, u0::AbstractVecOrMat, tspan, p::AbstractVector,
                              saveat::AbstractVector; kw...)
    sol, S = fwd_impl(h, u0, tspan, p, saveat, options(; kw...))
    function solve_tsit5_fwd_pullback(Δ)
        ū = unthunk(Δ)
        ū isa AbstractZero && return (NoTangent(), NoTangent(), NoTangent(), NoTangent(), ZeroTangent(), NoTangent())
        ub = reshape(ū, h.nin * size(u0, 2), 1, length(saveat))
        Sm = reshape(S, h.nin * size(u0, 2), h.P, length(saveat))
        dp = vec(sum(sum(Sm .* ub; dims = 1); dims = 3))       # Σ_j Σ_i ū_i(t_j) ∂u_i(t_j)/∂p
        return (NoTangent(), NoTangent(), NoTangent(), NoTangent(), ptangent(p, dp), NoTangent())
    end
    return sol, solve_tsit5_fwd_pullback
end

# --- the device-resident training loop (kanode_train_tsit5): n_iters iterations of LV_driver_KANODE.jl:279-291
# (forward solve, loss, InterpolatingAdjoint, Flux Adam, test-loss solve) in one kernel launch.  p, m, v, u0, target
# and the outputs are device pointers (upload / DevBuf); saveat lists are host vectors.  βp: Flux's running powers
# (opt.state[p][3]) on entry; advance them by the returned iteration count afterwards.
train_supported(h::Handle, B::Integer) = ccall(sym(:kanode_train_supported), Int32, (Ptr{Cvoid}, Int64), h.ptr, B) == 1
# λ of kanode_train_tsit5's L1 term (finite, >= 0; 0 = plain MSE).  kanode_train_forward_tsit5 refuses a non-zero one.
set_l1_penalty!(h::Handle, λ::Real) = check(h, ccall(sym(:kanode_set_l1_penalty), Cint, (Ptr{Cvoid}, Float64), h.ptr, λ))
l1_penalty(h::Handle) = ccall(sym(:kanode_get_l1_penalty), Float64, (Ptr{Cvoid},), h.ptr)
# KANODE_OPT_TRAIN_ANY_CHAIN (include/kanode.h): 1 = train_tsit5! also covers every other small fp64 chain whose solve
# and adjoint each run in one workgroup (a pruned [2,k,2], a [3,6,3] chain, three layers, up to 16 trajectories)
const OPT_TRAIN_ANY_CHAIN = Int32(21)
train_any_chain!(h::Handle, v::Integer = 1) = check(h, ccall(sym(:kanode_set_option), Cint, (Ptr{Cvoid}, Int32, Int64),
                                                             h.ptr, OPT_TRAIN_ANY_CHAIN, v))

"""train_tsit5!(h, p, m, v, u0, tspan, saveat, target, n_iters, loss; η, β, ϵ, βp, test, loss_test, grad, p_before,
counts, opt) -> (iters_done, stop_reason).  loss[it] is the loss at p_it (before the update), loss_test[it] at
p_{it+1}; test = (tf_test, saveat_test, target_test).  A stopped loop (stop_reason != 0: a kanode_train_stop)
returns normally with p, m, v as the last good iteration left them; any other failure throws.
l1: the weight λ of the sparsity term of sparse_on = 1 (LV_driver_KANODE.jl:187-201: loss + λ·Σ|p|, gradient +
λ·sign(p)), set on the handle for this call and restored afterwards.
Covered by default: one Lotka-Volterra trajectory (B = 1).  After train_any_chain!(h) (KANODE_OPT_TRAIN_ANY_CHAIN = 1)
also the other small fp64 chains, e.g. a pruned network, at B <= 16 trajectories: u0 is then N x B and target
N x B x n_save (column-major; the C side's [n_save][B][N])."""
function train_tsit5!(h::Handle, p::Ptr{Cvoid}, m::Ptr{Cvoid}, v::Ptr{Cvoid}, u0::Ptr{Cvoid}, tspan,
                      saveat::Vector{Float64}, target::Ptr{Cvoid}, n_iters::Integer, loss::Ptr{Cvoid};
                      η::Real = 1e-3, β = (0.9, 0.999), ϵ::Real = 1e-8, βp = β, test = nothing,
                      loss_test::Ptr{Cvoid} = C_NULL, grad::Ptr{Cvoid} = C_NULL, p_before::Ptr{Cvoid} = C_NULL,
                      counts::Ptr{Cvoid} = C_NULL, opt::SolverOptions = default_options(),
                      stream::Ptr{Cvoid} = C_NULL, l1::Real = 0.0, B::Integer = 1)
    train_supported(h, B) || throw(ArgumentError("train_tsit5!: not covered for this handle (train_any_chain!?)"))
    issorted(saveat) || throw(ArgumentError("saveat must be ascending"))
    tf_t, sv_t, tg_t = test === nothing ? (0.0, Float64[], Ptr{Cvoid}(C_NULL)) : (Float64(test[1]), Vector{Float64}(test[2]), test[3])
    done = Ref{Int64}(0)
    stop = Ref{Int32}(0)
    old = l1_penalty(h)
    set_l1_penalty!(h, l1)
    local st
    try
        st = GC.@preserve saveat sv_t ccall(sym(:kanode_train_tsit5), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Float64, Float64, Ptr{Float64}, Int64,
             Ptr{Cvoid}, Float64, Ptr{Float64}, Int64, Ptr{Cvoid}, Ref{SolverOptions}, Float64, Float64, Float64,
             Float64, Float64, Float64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int64},
             Ref{Int32}, Ptr{Cvoid}),
            h.ptr, p, m, v, u0, B, tspan[1], tspan[2], saveat, length(saveat), target, tf_t, sv_t, length(sv_t), tg_t,
            opt, η, β[1], β[2], ϵ, βp[1], βp[2], n_iters, loss, loss_test, grad, p_before, counts, done, stop, stream)
    finally
        set_l1_penalty!(h, old)
    end
    stop[] == 0 && check(h, st)
    return done[], stop[]
end

# --- the device-resident Fisher-KPP loop on the forward-mode gradient (kanode_train_forward_tsit5): n_iters
# iterations of Fisher-KPP_Source.jl:194-213 (tables, ForwardDiffSensitivity solve, loss, gradient, Flux Adam, the
# logged loss(p) solve) in one kernel launch, for the shapes of fsens_supported.  u0 is B x nx, target
# n_save x B x nx (device pointers); counts is n_iters x 4 (Int64: the sensitivity solve's naccept, nreject, then the
# logged-loss solve's, written only with a test problem: zero the buffer first).
train_forward_supported(h::Handle, B::Integer, with_test::Bool = false) =
    ccall(sym(:kanode_train_forward_supported), Int32, (Ptr{Cvoid}, Int64, Int32), h.ptr, B, with_test ? 1 : 0) == 1

"""train_forward_tsit5!(h, p, m, v, u0, B, tspan, saveat, target, n_iters, loss; η, β, ϵ, βp, test, loss_test, grad,
p_before, counts, opt) -> (iters_done, stop_reason): train_tsit5! for a small Fisher-KPP field of B trajectories.
loss[it] is the loss at p_it (before the update), loss_test[it] the logged loss at p_{it+1}; test = (tf_test,
saveat_test, target_test) needs train_forward_supported(h, B, true)."""
function train_forward_tsit5!(h::Handle, p::Ptr{Cvoid}, m::Ptr{Cvoid}, v::Ptr{Cvoid}, u0::Ptr{Cvoid}, B::Integer,
                              tspan, saveat::Vector{Float64}, target::Ptr{Cvoid}, n_iters::Integer,
                              loss::Ptr{Cvoid}; η::Real = 1e-2, β = (0.9, 0.999), ϵ::Real = 1e-8, βp = β,
                              test = nothing, loss_test::Ptr{Cvoid} = C_NULL, grad::Ptr{Cvoid} = C_NULL,
                              p_before::Ptr{Cvoid} = C_NULL, counts::Ptr{Cvoid} = C_NULL,
                              opt::SolverOptions = default_options(), stream::Ptr{Cvoid} = C_NULL)
    train_forward_supported(h, B, test !== nothing) ||
        throw(ArgumentError("train_forward_tsit5!: not covered for this handle"))
    issorted(saveat) || throw(ArgumentError("saveat must be ascending"))
    tf_t, sv_t, tg_t = test === nothing ? (0.0, Float64[], Ptr{Cvoid}(C_NULL)) : (Float64(test[1]), Vector{Float64}(test[2]), test[3])
    done = Ref{Int64}(0)
    stop = Ref{Int32}(0)
    st = GC.@preserve saveat sv_t ccall(sym(:kanode_train_forward_tsit5), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Float64, Float64, Ptr{Float64}, Int64,
         Ptr{Cvoid}, Float64, Ptr{Float64}, Int64, Ptr{Cvoid}, Ref{SolverOptions}, Float64, Float64, Float64, Float64,
         Float64, Float64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int64}, Ref{Int32},
         Ptr{Cvoid}),
        h.ptr, p, m, v, u0, B, tspan[1], tspan[2], saveat, length(saveat), target, tf_t, sv_t, length(sv_t), tg_t,
        opt, η, β[1], β[2], ϵ, βp[1], βp[2], n_iters, loss, loss_test, grad, p_before, counts, done, stop, stream)
    stop[] == 0 && check(h, st)
    return done[], stop[]
end

# --- ensemble training (kanode_train_ensemble_tsit5 / kanode_train_forward_ensemble_tsit5): R independent replicas
# of one problem in one launch, one workgroup each.  p, m, v are device pointers to R x P arrays (replica-major:
# Julia's P x R), the outputs carry a leading replica dimension (loss: n_iters x R in Julia's order); η, l1 and βp
# are host vectors of R entries (βp: R pairs).  A replica that stops does not throw: the returned vectors say which
# replicas stopped and why (kanode_train_stop); the others run on.
function train_ensemble_call(name::Symbol, h::Handle, R::Integer, p, m, v, u0, B::Integer, tspan,
                             saveat::Vector{Float64}, target, n_iters::Integer, loss, η, l1, β, ϵ, βp, test,
                             loss_test, grad, p_before, counts, opt::SolverOptions, stream)
    issorted(saveat) || throw(ArgumentError("saveat must be ascending"))
    ηv = η isa Real ? fill(Float64(η), R) : Vector{Float64}(η)
    l1v = l1 === nothing ? Float64[] : Vector{Float64}(l1)
    βv = βp === nothing ? repeat(Float64[β[1], β[2]], R) : Float64[x for pair in βp for x in pair]
    (length(ηv) == R && length(βv) == 2R && (l1 === nothing || length(l1v) == R)) ||
        throw(DimensionMismatch("η, l1 and βp need one entry per replica"))
    tf_t, sv_t, tg_t = test === nothing ? (0.0, Float64[], Ptr{Cvoid}(C_NULL)) : (Float64(test[1]), Vector{Float64}(test[2]), test[3])
    done = zeros(Int64, R)
    stop = zeros(Int32, R)
    st = GC.@preserve saveat sv_t ηv l1v βv done stop ccall(sym(name), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Float64, Float64, Ptr{Float64}, Int64,
         Ptr{Cvoid}, Float64, Ptr{Float64}, Int64, Ptr{Cvoid}, Ref{SolverOptions}, Ptr{Float64}, Ptr{Float64}, Float64,
         Float64, Float64, Ptr{Float64}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64},
         Ptr{Int32}, Ptr{Cvoid}),
        h.ptr, R, p, m, v, u0, B, tspan[1], tspan[2], saveat, length(saveat), target, tf_t, sv_t, length(sv_t), tg_t,
        opt, ηv, l1 === nothing ? Ptr{Float64}(C_NULL) : pointer(l1v), β[1], β[2], ϵ, βv, n_iters, loss, loss_test,
        grad, p_before, counts, done, stop, stream)
    check(h, st)
    return done, stop
end

"""train_ensemble_tsit5!(h, R, p, m, v, u0, tspan, saveat, target, n_iters, loss; η, l1, β, ϵ, βp, test, loss_test,
grad, p_before, counts, opt) -> (iters_done, stop_reason), vectors of R: train_tsit5! on R replicas at once.  η and
l1 are a number or R of them (l1 = nothing: no penalty; the handle's set_l1_penalty! value is not read), βp R pairs of
running powers (nothing: a fresh optimiser); advance replica r's by iters_done[r] products afterwards."""
function train_ensemble_tsit5!(h::Handle, R::Integer, p::Ptr{Cvoid}, m::Ptr{Cvoid}, v::Ptr{Cvoid}, u0::Ptr{Cvoid},
                               tspan, saveat::Vector{Float64}, target::Ptr{Cvoid}, n_iters::Integer, loss::Ptr{Cvoid};
                               η = 1e-3, l1 = nothing, β = (0.9, 0.999), ϵ::Real = 1e-8, βp = nothing, test = nothing,
                               loss_test::Ptr{Cvoid} = C_NULL, grad::Ptr{Cvoid} = C_NULL,
                               p_before::Ptr{Cvoid} = C_NULL, counts::Ptr{Cvoid} = C_NULL,
                               opt::SolverOptions = default_options(), stream::Ptr{Cvoid} = C_NULL)
    train_supported(h, 1) || throw(ArgumentError("train_ensemble_tsit5!: not covered for this handle"))
    l1v = l1 isa Real ? fill(Float64(l1), R) : l1
    return train_ensemble_call(:kanode_train_ensemble_tsit5, h, R, p, m, v, u0, 1, tspan, saveat, target, n_iters, loss,
                               η, l1v, β, ϵ, βp, test, loss_test, grad, p_before, counts, opt, stream)
end

# the ensemble of every other small chain (kanode_fit_ensemble_tsit5): a pruned [2,k,2], [3,6,3], three layers, up to
# 16 initial conditions; never the Lotka-Volterra shape, which train_ensemble_tsit5! keeps
fit_ensemble_supported(h::Handle, B::Integer) =
    ccall(sym(:kanode_fit_ensemble_supported), Int32, (Ptr{Cvoid}, Int64), h.ptr, B) == 1

"""fit_ensemble_tsit5!(h, R, p, m, v, u0, B, tspan, saveat, target, n_iters, loss; η, l1, β, ϵ, βp, test, loss_test,
grad, p_before, counts, opt) -> (iters_done, stop_reason), vectors of R: train_ensemble_tsit5! for the small chains
train_tsit5! covers only after train_any_chain! (the option is not read: this call is the opt-in), at B trajectories.
Replica r equals train_tsit5! on that handle, bit for bit.  The arguments are train_ensemble_tsit5!'s."""
function fit_ensemble_tsit5!(h::Handle, R::Integer, p::Ptr{Cvoid}, m::Ptr{Cvoid}, v::Ptr{Cvoid}, u0::Ptr{Cvoid},
                             B::Integer, tspan, saveat::Vector{Float64}, target::Ptr{Cvoid}, n_iters::Integer,
                             loss::Ptr{Cvoid}; η = 1e-3, l1 = nothing, β = (0.9, 0.999), ϵ::Real = 1e-8, βp = nothing,
                             test = nothing, loss_test::Ptr{Cvoid} = C_NULL, grad::Ptr{Cvoid} = C_NULL,
                             p_before::Ptr{Cvoid} = C_NULL, counts::Ptr{Cvoid} = C_NULL,
                             opt::SolverOptions = default_options(), stream::Ptr{Cvoid} = C_NULL)
    fit_ensemble_supported(h, B) ||
        throw(ArgumentError("fit_ensemble_tsit5!: not covered for this handle (the Lotka-Volterra shape: train_ensemble_tsit5!)"))
    l1v = l1 isa Real ? fill(Float64(l1), R) : l1
    return train_ensemble_call(:kanode_fit_ensemble_tsit5, h, R, p, m, v, u0, B, tspan, saveat, target, n_iters, loss,
                               η, l1v, β, ϵ, βp, test, loss_test, grad, p_before, counts, opt, stream)
end

"""train_forward_ensemble_tsit5!(h, R, p, m, v, u0, B, tspan, saveat, target, n_iters, loss; ...) ->
(iters_done, stop_reason): train_forward_tsit5! on R replicas at once (no L1 term)."""
function train_forward_ensemble_tsit5!(h::Handle, R::Integer, p::Ptr{Cvoid}, m::Ptr{Cvoid}, v::Ptr{Cvoid},
                                       u0::Ptr{Cvoid}, B::Integer, tspan, saveat::Vector{Float64}, target::Ptr{Cvoid},
                                       n_iters::Integer, loss::Ptr{Cvoid}; η = 1e-2, β = (0.9, 0.999), ϵ::Real = 1e-8,
                                       βp = nothing, test = nothing, loss_test::Ptr{Cvoid} = C_NULL,
                                       grad::Ptr{Cvoid} = C_NULL, p_before::Ptr{Cvoid} = C_NULL,
                                       counts::Ptr{Cvoid} = C_NULL, opt::SolverOptions = default_options(),
                                       stream::Ptr{Cvoid} = C_NULL)
    train_forward_supported(h, B, test !== nothing) ||
        throw(ArgumentError("train_forward_ensemble_tsit5!: not covered for this handle"))
    return train_ensemble_call(:kanode_train_forward_ensemble_tsit5, h, R, p, m, v, u0, B, tspan, saveat, target,
                               n_iters, loss, η, nothing, β, ϵ, βp, test, loss_test, grad, p_before, counts, opt, stream)
end

# --- the ensemble solve (kanode_solve_ensemble_tsit5): the forward solve of one problem at R parameter vectors in one
# launch, one workgroup per replica: what an ensemble trained, a parameter sweep, a loss landscape.
solve_ensemble_supported(h::Handle, B::Integer) =
    ccall(sym(:kanode_solve_ensemble_supported), Int32, (Ptr{Cvoid}, Int64), h.ptr, B) == 1

"""solve_ensemble_tsit5(h, u0, tspan, ps, saveat; abstol, reltol, dt, adaptive, ...) -> (sol, stats, stop).
ps is [P, R]: column r holds replica r's parameters (the C side's replica-major [R][P]).  sol is [N, n_save, R] for a
vector u0 and [N, B, n_save, R] for a matrix, filled with NaN beforehand; stats a vector of R SolveStats; stop[r] is 0,
or 1 where replica r reached maxiters (a kanode_solve_stop: it does not throw, and its columns past the last stop it
reached stay NaN).  Covered: solve_ensemble_supported(h, B), i.e. where solve_tsit5 runs as one workgroup."""
function solve_ensemble_tsit5(h::Handle, u0::AbstractVecOrMat, tspan, ps::AbstractMatrix, saveat::AbstractVector; kw...)
    size(ps, 1) == h.P || throw(DimensionMismatch("ps has $(size(ps, 1)) rows, the handle $(h.P) parameters"))
    checku(h, u0, h.nin, "u0")
    h.nin == h.nout || throw(ArgumentError("an ODE RHS needs a chain with in_dims == out_dims"))
    T = h.T
    R, B = size(ps, 2), size(u0, 2)
    1 <= R <= 4096 || throw(ArgumentError("solve_ensemble_tsit5: 1 <= R <= 4096 replicas"))
    ts = Vector{Float64}(saveat)
    (issorted(ts) && !isempty(ts)) || throw(ArgumentError("saveat must be ascending and not empty"))
    solve_ensemble_supported(h, B) || throw(ArgumentError("solve_ensemble_tsit5: not covered for this handle / batch"))
    opt = options(; kw...)
    pd, ud = upload(tohost(T, ps)), upload(tohost(T, u0))
    out = fill(T(NaN), h.nin, B, length(ts), R)
    od = upload(out)
    stats = Vector{SolveStats}(undef, R)
    stop = zeros(Int32, R)
    st = GC.@preserve ts stats stop ccall(sym(:kanode_solve_ensemble_tsit5), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Float64, Float64, Ptr{Float64}, Int64, Ptr{Cvoid},
         Ref{SolverOptions}, Ptr{SolveStats}, Ptr{Int32}, Ptr{Cvoid}),
        h.ptr, R, pd.ptr, ud.ptr, B, tspan[1], tspan[2], ts, length(ts), od.ptr, opt, stats, stop, C_NULL)
    check(h, st)
    download!(out, od)
    sol = u0 isa AbstractVector ? reshape(out, h.nin, length(ts), R) : out
    return sol, stats, stop
end

# --- the trajectory ensemble (kanode_solve_trajectories_tsit5): the forward solves of one problem at one p from R
# initial conditions in one launch, every trajectory an ODE of its own (EnsembleProblem over u0): a trained network
# on held-out initial conditions, a phase portrait, generated data.
solve_trajectories_supported(h::Handle) =
    ccall(sym(:kanode_solve_trajectories_supported), Int32, (Ptr{Cvoid},), h.ptr) == 1

"""solve_trajectories(h, u0, tspan, p, saveat; abstol, reltol, dt, adaptive, ...) -> (sol, stats, stop).
u0 is [N, R]: column r holds trajectory r's initial condition (the C side's [R][N]).  Every trajectory is solved on its
own, with its own error norm, step sizes and rejections, as solve_tsit5 solves u0[:, r] alone, bit for bit, where
solve_tsit5 with the matrix u0 solves ONE ODE over all N*R entries.  sol is [N, R, n_save], the layout solve_tsit5 gives
that matrix, filled with NaN beforehand; stats a vector of R SolveStats; stop[r] is 0, or 1 where trajectory r reached
maxiters (a kanode_solve_stop: it does not throw, and its columns past the last stop it reached stay NaN).  Up to 65536
trajectories per call.  Covered: solve_trajectories_supported(h), i.e. chains where solve_tsit5 runs as one workgroup
at one trajectory."""
function solve_trajectories(h::Handle, u0::AbstractMatrix, tspan, p::AbstractVector, saveat::AbstractVector; kw...)
    checkp(h, p)
    checku(h, u0, h.nin, "u0")
    h.nin == h.nout || throw(ArgumentError("an ODE RHS needs a chain with in_dims == out_dims"))
    T = h.T
    R = size(u0, 2)
    1 <= R <= 65536 || throw(ArgumentError("solve_trajectories: 1 <= R <= 65536 trajectories"))
    ts = Vector{Float64}(saveat)
    (issorted(ts) && !isempty(ts)) || throw(ArgumentError("saveat must be ascending and not empty"))
    solve_trajectories_supported(h) || throw(ArgumentError("solve_trajectories: not covered for this handle"))
    opt = options(; kw...)
    pd, ud = upload(tohost(T, p)), upload(tohost(T, u0))
    out = fill(T(NaN), h.nin, R, length(ts))
    od = upload(out)
    stats = Vector{SolveStats}(undef, R)
    stop = zeros(Int32, R)
    st = GC.@preserve ts stats stop ccall(sym(:kanode_solve_trajectories_tsit5), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Float64, Float64, Ptr{Float64}, Int64, Ptr{Cvoid},
         Ref{SolverOptions}, Ptr{SolveStats}, Ptr{Int32}, Ptr{Cvoid}),
        h.ptr, pd.ptr, ud.ptr, R, tspan[1], tspan[2], ts, length(ts), od.ptr, opt, stats, stop, C_NULL)
    check(h, st)
    download!(out, od)
    return out, stats, stop
end

# --- the gradient of a trajectory ensemble (kanode_trajectories_gradient_tsit5): the loss mean((u - target)^2) over R
# trajectories of one problem at one p and its gradient, every trajectory an ODE of its own with its own forward and
# adjoint step control, one workgroup each; multi-trajectory training with one controller per trajectory.
trajectories_gradient_supported(h::Handle) =
    ccall(sym(:kanode_trajectories_gradient_supported), Int32, (Ptr{Cvoid},), h.ptr) == 1

"""trajectories_gradient(h, u0, tspan, p, saveat, target; abstol, reltol, dt, adaptive, ...) ->
(loss, dp, dp_rows, loss_rows, fwd_stats, adj_stats, stop).
u0 is [N, R] (column r: trajectory r's initial condition), target [N, R, n_save], the layout solve_trajectories
returns.  loss is the mean over the whole tensor, dp [P] its gradient: the mean of the R batch-1 gradients dp_rows
[P, R], both summed in an order that depends on R alone (chunks of 64 trajectories).  stop[r] is 0 or a
kanode_train_stop; a stopped trajectory does not throw: its column of dp_rows, its loss_rows entry, loss and dp are NaN.
Float64 handles only; up to 65536 trajectories per call.  Covered: trajectories_gradient_supported(h).  The handle's L1
penalty is not read."""
function trajectories_gradient(h::Handle, u0::AbstractMatrix, tspan, p::AbstractVector, saveat::AbstractVector,
                               target::AbstractArray{<:Real,3}; kw...)
    checkp(h, p)
    checku(h, u0, h.nin, "u0")
    h.nin == h.nout || throw(ArgumentError("an ODE RHS needs a chain with in_dims == out_dims"))
    T = h.T
    T == Float64 || throw(ArgumentError("trajectories_gradient: Float64 handles only"))
    R = size(u0, 2)
    1 <= R <= 65536 || throw(ArgumentError("trajectories_gradient: 1 <= R <= 65536 trajectories"))
    ts = Vector{Float64}(saveat)
    (issorted(ts) && !isempty(ts)) || throw(ArgumentError("saveat must be ascending and not empty"))
    size(target) == (h.nin, R, length(ts)) ||
        throw(DimensionMismatch("target is $(size(target)); expected $((h.nin, R, length(ts)))"))
    trajectories_gradient_supported(h) || throw(ArgumentError("trajectories_gradient: not covered for this handle"))
    opt = options(; kw...)
    pd, ud, xd = upload(tohost(T, p)), upload(tohost(T, u0)), upload(tohost(T, target))
    dp, rows, lrows = zeros(T, h.P), zeros(T, h.P, R), zeros(T, R)
    dpd, rowsd, lrowsd = upload(dp), upload(rows), upload(lrows)
    loss = Ref{Float64}(NaN)
    fst = Vector{SolveStats}(undef, R)
    ast = Vector{SolveStats}(undef, R)
    stop = zeros(Int32, R)
    st = GC.@preserve ts fst ast stop ccall(sym(:kanode_trajectories_gradient_tsit5), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Float64, Float64, Ptr{Float64}, Int64, Ptr{Cvoid},
         Ref{SolverOptions}, Ref{Float64}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},
         Ptr{SolveStats}, Ptr{SolveStats}, Ptr{Int32}, Ptr{Cvoid}),
        h.ptr, pd.ptr, ud.ptr, R, tspan[1], tspan[2], ts, length(ts), xd.ptr, opt, loss, dpd.ptr, rowsd.ptr,
        lrowsd.ptr, C_NULL, C_NULL, fst, ast, stop, C_NULL)
    check(h, st)
    download!(dp, dpd)
    download!(rows, rowsd)
    download!(lrows, lrowsd)
    return loss[], dp, rows, lrows, fst, ast, stop
end

# --- the same gradient on a Float32 handle (kanode_trajectories_gradient_f32_tsit5): float arrays, the total widened
trajectories_gradient_f32_supported(h::Handle) =
    ccall(sym(:kanode_trajectories_gradient_f32_supported), Int32, (Ptr{Cvoid},), h.ptr) == 1

"""trajectories_gradient_f32(h, u0, tspan, p, saveat, target; kw...) -> trajectories_gradient's tuple on a Float32
handle: dp, dp_rows and loss_rows are Float32, loss is the Float32 total as a Float64.  Covered:
trajectories_gradient_f32_supported(h) (Float32 small chains with an even parameter count).  The handle's L1 penalty is
not read."""
function trajectories_gradient_f32(h::Handle, u0::AbstractMatrix, tspan, p::AbstractVector, saveat::AbstractVector,
                                   target::AbstractArray{<:Real,3}; kw...)
    checkp(h, p)
    checku(h, u0, h.nin, "u0")
    h.nin == h.nout || throw(ArgumentError("an ODE RHS needs a chain with in_dims == out_dims"))
    T = h.T
    T == Float32 || throw(ArgumentError("trajectories_gradient_f32: Float32 handles only"))
    R = size(u0, 2)
    1 <= R <= 65536 || throw(ArgumentError("trajectories_gradient_f32: 1 <= R <= 65536 trajectories"))
    ts = Vector{Float64}(saveat)
    (issorted(ts) && !isempty(ts)) || throw(ArgumentError("saveat must be ascending and not empty"))
    size(target) == (h.nin, R, length(ts)) ||
        throw(DimensionMismatch("target is $(size(target)); expected $((h.nin, R, length(ts)))"))
    trajectories_gradient_f32_supported(h) ||
        throw(ArgumentError("trajectories_gradient_f32: not covered for this handle"))
    opt = options(; kw...)
    pd, ud, xd = upload(tohost(T, p)), upload(tohost(T, u0)), upload(tohost(T, target))
    dp, rows, lrows = zeros(T, h.P), zeros(T, h.P, R), zeros(T, R)
    dpd, rowsd, lrowsd = upload(dp), upload(rows), upload(lrows)
    loss = Ref{Float64}(NaN)
    fst = Vector{SolveStats}(undef, R)
    ast = Vector{SolveStats}(undef, R)
    stop = zeros(Int32, R)
    st = GC.@preserve ts fst ast stop ccall(sym(:kanode_trajectories_gradient_f32_tsit5), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Float64, Float64, Ptr{Float64}, Int64, Ptr{Cvoid},
         Ref{SolverOptions}, Ref{Float64}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},
         Ptr{SolveStats}, Ptr{SolveStats}, Ptr{Int32}, Ptr{Cvoid}),
        h.ptr, pd.ptr, ud.ptr, R, tspan[1], tspan[2], ts, length(ts), xd.ptr, opt, loss, dpd.ptr, rowsd.ptr,
        lrowsd.ptr, C_NULL, C_NULL, fst, ast, stop, C_NULL)
    check(h, st)
    download!(dp, dpd)
    download!(rows, rowsd)
    download!(lrows, lrowsd)
    return loss[], dp, rows, lrows, fst, ast, stop
end

# --- pruning a sparsified KAN (LV_driver_KANODE.jl:52-108): per-edge scores on the device, the keep rule and the
# parameter slicing on the host.  Scores are Julia [O, I] matrices (the memory kanode_edge_scores writes).
layer_length(h::Handle, i::Integer) = Int(ccall(sym(:kanode_layer_param_length), Int64, (Ptr{Cvoid}, Int32), h.ptr, i))

"""edge_scores(l, x, p) -> [scores_1, scores_2, ..]: scores_i[o, j] = max_k |φ_{o,j}(x_k)| of layer i, x [I, K]
propagated through the layers with kanode_layer_forward (Activation_getter.jl:39).  The quantity prune reads from
activation_getter (:79-80), without the per-sample arrays; a NaN activation makes its edge's score NaN."""
function edge_scores(l::KANChainHip, x::AbstractMatrix, p::AbstractVector)
    h = l.h
    checkp(h, p)
    checku(h, x, h.nin, "x")
    T = h.T
    K = size(x, 2)
    K >= 1 || throw(ArgumentError("edge_scores needs at least one sample"))
    pd, xd = upload(tohost(T, p)), upload(tohost(T, x))
    out = Matrix{T}[]
    off = 0
    sig = (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid})
    for (i, s) in enumerate(l.specs)
        sc = Matrix{T}(undef, Int(s.out_dims), Int(s.in_dims))
        sd = DevBuf(sizeof(sc))
        pl = pd.ptr + off * sizeof(T)
        GC.@preserve pd xd sd check(h, ccall(sym(:kanode_edge_scores), Cint, sig, h.ptr, i - 1, pl, xd.ptr, sd.ptr, K,
                                             C_NULL))
        push!(out, download!(sc, sd))
        if i < length(l.specs)
            yd = DevBuf(Int(s.out_dims) * K * sizeof(T))
            GC.@preserve pd xd yd check(h, ccall(sym(:kanode_layer_forward), Cint, sig, h.ptr, i - 1, pl, xd.ptr,
                                                 yd.ptr, K, C_NULL))
            hipcheck(ccall((:hipDeviceSynchronize, HIPLIB), Cint, ()), "hipDeviceSynchronize")
            xd = yd
        end
        off += layer_length(h, i - 1)
    end
    return out
end

"""prune_nodes(scores, θ) -> kept: for every hidden layer the nodes j with
min(max_i scores_l[j, i], max_o scores_{l+1}[o, j]) > θ (:79-83), all scores taken on the unpruned network."""
function prune_nodes(scores::AbstractVector, θ::Real)
    length(scores) >= 2 || throw(ArgumentError("prune needs a chain of at least 2 layers"))
    all(s -> all(isfinite, s), scores) || throw(ArgumentError("prune: a score is not finite"))
    kept = Vector{Int}[]
    for l in 1:(length(scores) - 1)
        in_score = vec(maximum(scores[l]; dims = 2))
        out_score = vec(maximum(scores[l + 1]; dims = 1))
        k = findall(min.(in_score, out_score) .> θ)
        isempty(k) && throw(ArgumentError("prune: every node of hidden layer $l scores at most θ"))
        push!(kept, k)
    end
    return kept
end

"""prune(l, p, x; theta = 1e-2) -> (l_pruned, p_pruned, kept): the narrower chain and its flat parameters.  Layer i
keeps the rows kept[i] of C and W, layer i + 1 the column blocks g + G·(j - 1) of C and the columns j of W for j in
kept[i].  Unlike the reference's prune (which slices the freshly initialised global pM, :96-104, and fills layer 2's
W from its C, :104) the kept nodes keep their trained C and W."""
function prune(l::KANChainHip, p::AbstractVector, x::AbstractMatrix; theta::Real = 1e-2, device::Integer = 0)
    kept = prune_nodes(edge_scores(l, x, p), theta)
    specs, pp = LayerSpec[], eltype(p)[]
    off = 0
    n = length(l.specs)
    for (i, s) in enumerate(l.specs)
        I, O, G = Int(s.in_dims), Int(s.out_dims), Int(s.grid_len)
        rows = i < n ? kept[i] : collect(1:O)
        ins = i > 1 ? kept[i - 1] : collect(1:I)
        cols = vec([g + G * (j - 1) for g in 1:G, j in ins])
        C = reshape(p[(off + 1):(off + O * G * I)], O, G * I)
        off += O * G * I
        append!(pp, vec(C[rows, cols]))
        if s.use_base_act == 1
            W = reshape(p[(off + 1):(off + O * I)], O, I)
            off += O * I
            append!(pp, vec(W[rows, ins]))
        end
        push!(specs, LayerSpec(Int32(length(ins)), Int32(length(rows)), s.grid_len, s.normalizer, s.basis,
                               s.use_base_act, s.grid_lo, s.grid_hi, s.denominator, s.iqf_reference_quirk))
    end
    return KANChainHip(specs; T = l.h.T, device), pp, kept
end

# --- data-parallel training across GPUs (kanode_comm_*): one process per GPU, each with its trajectory
# shard; after the adjoint, the flat [dp; L] (device) is SUM all-reduced over RCCL and the mean applied by
# kanode_adam_step(scale = 1/nranks).  Rank 0 calls comm_unique_id() and the host distributes the bytes
# (MPI.bcast, a file); every rank then calls Comm(nranks, rank, id, device) (collective).
const COMM_ID_BYTES = 128
function comm_unique_id()
    id = zeros(UInt8, COMM_ID_BYTES)
    st = ccall(sym(:kanode_comm_unique_id), Cint, (Ptr{UInt8},), id)
    st == 0 || error("libkanode: ", unsafe_string(ccall(sym(:kanode_comm_last_error), Cstring, (Ptr{Cvoid},), C_NULL)))
    return id
end
mutable struct Comm
    ptr::Ptr{Cvoid}
    nranks::Int
    rank::Int
end
function Comm(nranks::Integer, rank::Integer, id::Vector{UInt8}, device::Integer)
    length(id) == COMM_ID_BYTES || throw(ArgumentError("the unique id is $COMM_ID_BYTES bytes"))
    out = Ref{Ptr{Cvoid}}(C_NULL)
    st = ccall(sym(:kanode_comm_create), Cint, (Int32, Int32, Ptr{UInt8}, Int32, Ref{Ptr{Cvoid}}),
               nranks, rank, id, device, out)
    st == 0 || error("libkanode: ", unsafe_string(ccall(sym(:kanode_comm_last_error), Cstring, (Ptr{Cvoid},), C_NULL)))
    c = Comm(out[], Int(nranks), Int(rank))
    finalizer(x -> (x.ptr == C_NULL || ccall(sym(:kanode_comm_destroy), Cvoid, (Ptr{Cvoid},), x.ptr)), c)
    return c
end
"""allreduce_sum!(c, buf, count, T; stream): buf (device, count entries of T) <- Σ over the ranks, in place."""
function allreduce_sum!(c::Comm, buf::Ptr{Cvoid}, count::Integer, ::Type{T}; stream::Ptr{Cvoid} = C_NULL) where {T}
    haskey(DTYPE, T) || throw(ArgumentError("the all-reduce takes Float32 or Float64, not $T"))
    st = ccall(sym(:kanode_comm_allreduce_sum), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Ptr{Cvoid}),
               c.ptr, buf, count, DTYPE[T], stream)
    st == 0 || error("libkanode: ", unsafe_string(ccall(sym(:kanode_comm_last_error), Cstring, (Ptr{Cvoid},), c.ptr)))
    return buf
end

end # module
