"""The native integrator (kanode_solve_tsit5 / kanode_adjoint_tsit5) vs the Python statement of
the same algorithm (kanode/ode.py, kanode/adjoint.py with native=False) driving the same HIP
RHS, and vs the CPU oracle: identical step sequences, saveat values and gradients.
(solve(prob, Tsit5(); saveat) at LV_driver_KANODE.jl:180-184, Fisher-KPP_Source.jl:102-103;
InterpolatingAdjoint = the NeuralODE default sensealg.)"""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from gpu_util import device, t
from oracle import oracle as O
from oracle_rhs import OracleFKRHS

import kanode
from kanode import _lib as L

pytestmark = pytest.mark.gpu


def fk(nx, table=None):
    kan1 = kanode.Chain(kanode.KDense(1, 1, 10, normalizer="softsign"))
    return kanode.FisherKPPRHS(kan1, nx=nx, dx=1.0 / (nx - 1), D=0.01, device=device(), table=table)


def lv(dtype=torch.float64):
    return kanode.ChainRHS(kanode.Chain(kanode.KDense(2, 10, 5), kanode.KDense(10, 2, 5)), dtype=dtype,
                           device=device())


def fk_u0(nx, B, seed=0):
    rng = np.random.default_rng(seed)
    x = np.arange(nx) / (nx - 1)
    c, d, a = rng.uniform(0.3, 0.7, (B, 1)), rng.uniform(0.1, 0.3, (B, 1)), rng.uniform(0.5, 1, (B, 1))
    return a * (np.tanh((x - (c - d / 2)) / (d / 10)) - np.tanh((x - (c + d / 2)) / (d / 10))) / 2


CASES = {
    "fk256": (lambda: fk(256), lambda: fk_u0(256, 4), 11, 1.0, (0.0, 2.0), [0.25 * i for i in range(9)]),
    "fk256_rec": (lambda: fk(256, False), lambda: fk_u0(256, 3, 1), 11, 1.0, (0.0, 1.0), [0.0, 0.3, 0.3, 1.0]),
    "fk26": (lambda: fk(26), lambda: fk_u0(26, 1, 2), 11, 1.0, (0.0, 2.0), [0.5 * i for i in range(5)]),
    "lv64": (lv, lambda: np.array([[1.0, 1.0], [0.7, 1.3], [1.5, 0.6]]), 240, 0.3, (0.0, 3.5),
             [0.1 * i for i in range(35)]),
    "lv32": (lambda: lv(torch.float32), lambda: np.random.default_rng(3).uniform(0.5, 2.0, (64, 2)), 240, 0.3,
             (0.0, 3.5), [0.1 * i for i in range(35)]),
}


def _setup(name):
    make, mk_u0, P, scale, tspan, ts = CASES[name]
    rhs = make()
    dt = rhs.hd.dtype
    p = t(np.random.default_rng(7).uniform(-scale, scale, P), dt)
    return rhs, t(mk_u0(), dt), p, tspan, ts


def _tol(dtype):
    return 1e-11 if dtype == torch.float64 else 2e-5


# fixed steps inside the explicit stability limit (FK256: D/dx² = 650)
FIXED = {"fk256": ((0.0, 0.2), 5e-4), "fk256_rec": ((0.0, 0.2), 5e-4)}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("adaptive", [True, False])
def test_native_forward_matches_python_driver(name, adaptive):
    rhs, u0, p, tspan, ts = _setup(name)
    dt = 0.01
    if not adaptive and name in FIXED:
        tspan, dt = FIXED[name]
        ts = [x for x in ts if x <= tspan[1]] + [tspan[1]]
    f64 = u0.dtype == torch.float64
    opt = kanode.Tsit5Options(adaptive=adaptive, dt=None if adaptive else dt, abstol=1e-8 if f64 else 1e-6,
                              reltol=1e-7 if f64 else 1e-4)
    nat = kanode.solve(rhs, u0, tspan, p, ts, opt)
    py = kanode.solve(rhs, u0, tspan, p, ts, dataclasses.replace(opt, native=False))
    assert nat.u.shape == py.u.shape
    scale = max(1.0, py.u.abs().max().item())
    if f64 or not adaptive:
        assert nat.stats["naccept"] == py.stats["naccept"] and nat.stats["nreject"] == py.stats["nreject"]
        assert nat.stats["nf"] == py.stats["nf"]
        # adaptive, device step control: the controller's pow() on the GPU may differ from the host's
        # libm in the last ulp, so dt can differ in its last bits: 1e-3 of the tolerance
        tol = max(_tol(u0.dtype), 1e-3 * opt.reltol if adaptive else 0.0)
        assert (nat.u - py.u).abs().max().item() <= tol * scale
    else:
        # fp32 adaptive: the Hairer-Wanner initial-step norms round differently (native: double
        # accumulation, Python: fp32 tensors), so the step sequences may differ; both meet reltol
        assert abs(nat.stats["naccept"] - py.stats["naccept"]) <= 2
        assert (nat.u - py.u).abs().max().item() <= 20 * opt.reltol * scale


@pytest.mark.parametrize("name", ["fk256", "fk26", "lv64"])
def test_native_adjoint_matches_python_adjoint(name):
    rhs, u0, p0, tspan, ts = _setup(name)
    w = t(np.random.default_rng(11).normal(size=(len(ts),) + tuple(u0.shape)), u0.dtype)
    # fp32: a reltol near the fp32 rounding level would make both controllers follow rounding noise
    opt = kanode.Tsit5Options(abstol=1e-8, reltol=1e-7) if u0.dtype == torch.float64 else \
        kanode.Tsit5Options(abstol=1e-6, reltol=1e-4)
    out = []
    for native in (True, False):
        p = p0.clone().requires_grad_(True)
        x0 = u0.clone().requires_grad_(True)
        sol = kanode.solve(rhs, x0, tspan, p, ts, dataclasses.replace(opt, native=native),
                           sensealg="interpolating_adjoint")
        gp, gu = torch.autograd.grad((sol.u * w).sum(), [p, x0])
        out.append((gp, gu, sol.stats))
    (gp, gu, sn), (rp, ru, sp) = out
    assert sn["naccept"] == sp["naccept"]
    na, nb = sn["adjoint"]["naccept"], sp["adjoint"]["naccept"]
    # The two drivers sum the [λ; μ] error norm in different orders (native: the fused step's wave and
    # block partials; Python: per-stage launches), so their step sizes agree to the norm's rounding.
    # FK256's adjoint is stability-limited (~2000 steps hovering at EEst ~ 1), where those last-bit
    # step differences are carried to ~1e-8 even with equal step counts: compared at the tolerance.
    stiff = name == "fk256"
    if na == nb and sn["adjoint"]["nreject"] == sp["adjoint"]["nreject"] and not stiff:
        tol = 1e-9 if u0.dtype == torch.float64 else 1e-3      # same step sequence: rounding only
    else:
        # A stability-limited adjoint (FK256: ~2000 steps hovering at EEst ~ 1) can flip one
        # accept/reject on last-bit differences of the norm (fma vs separate rounding); the two
        # then integrate the same ODE on different step sequences, so they agree to the tolerance.
        # fp32: the initial-step norms differ at fp32 rounding (the native norms accumulate in
        # double), so the step sequences may differ from the start.
        assert abs(na - nb) <= (0.01 if u0.dtype == torch.float64 else 0.1) * nb
        tol = 50 * opt.reltol if u0.dtype == torch.float64 else 5e-3
    assert (gp - rp).abs().max().item() <= tol * rp.abs().max().item()
    assert (gu - ru).abs().max().item() <= tol * ru.abs().max().item()


def test_native_adjoint_fp32_matches_fp64():
    """LV in fp32 (BASELINE configs[1]'s dtype): the native solve + adjoint gradient agrees with the
    fp64 native gradient of the same problem to the fp32 / reltol level."""
    grads = []
    for dtype in (torch.float32, torch.float64):
        rhs = lv(dtype)
        u0 = t(np.random.default_rng(3).uniform(0.5, 2.0, (64, 2)), dtype)
        p = t(np.random.default_rng(7).uniform(-0.3, 0.3, 240), dtype).requires_grad_(True)
        ts = [0.1 * i for i in range(35)]
        w = t(np.random.default_rng(11).normal(size=(35, 64, 2)), dtype)
        sol = kanode.solve(rhs, u0, (0.0, 3.5), p, ts, kanode.Tsit5Options(abstol=1e-6, reltol=1e-5),
                           sensealg="interpolating_adjoint")
        (g,) = torch.autograd.grad((sol.u * w).sum(), [p])
        grads.append(g.double())
    assert (grads[0] - grads[1]).abs().max().item() <= 2e-3 * grads[1].abs().max().item()


def test_native_fk26_solve_and_gradient_match_cpu_oracle():
    """End to end against the oracle: the native GPU solve + adjoint vs the Python driver on the
    plain-C restatement of rc_kanode (dense Laplacian matvec, Fisher-KPP_Source.jl:55-59,95-98)."""
    rhs, u0, p0, tspan, ts = _setup("fk26")
    cpu = OracleFKRHS(O.LayerSpec(1, 1, 10, "softsign"), 0.01, 1.0 / 25, dense=True)
    w = np.random.default_rng(2).normal(size=(len(ts),) + tuple(u0.shape))
    opt = kanode.Tsit5Options(abstol=1e-9, reltol=1e-9)
    res = []
    for f, dev in ((rhs, device()), (cpu, "cpu")):
        p = p0.detach().to(dev).clone().requires_grad_(True)
        sol = kanode.solve(f, u0.to(dev), tspan, p, ts, opt, sensealg="interpolating_adjoint")
        (g,) = torch.autograd.grad((sol.u * torch.as_tensor(w, device=dev)).sum(), [p])
        res.append((sol.u.detach().cpu(), g.cpu(), sol.stats))
    (ug, gg, sg), (uc, gc, sc) = res
    assert sg["naccept"] == sc["naccept"] and sg["adjoint"]["naccept"] == sc["adjoint"]["naccept"]
    assert (ug - uc).abs().max().item() <= 1e-11
    assert (gg - gc).abs().max().item() <= 1e-9 * gc.abs().max().item()


def test_native_surrogate_pair_solve_and_gradient_match_cpu_oracle():
    """The Burgers surrogate KAN [41, 10, 41] G=5 (Burgers_Surrogate.jl:85-97 at its 41 points: a
    wide-in + wide-out pair, whose stages form their inputs inside the wide-in kernel and write dp
    with =) through the native solve + InterpolatingAdjoint, against the Python driver on the oracle
    chain on the CPU."""
    from oracle_rhs import OracleChainRHS
    specs = [O.LayerSpec(41, 10, 5, "softsign"), O.LayerSpec(10, 41, 5, "softsign")]
    chain = kanode.Chain(kanode.KDense(41, 10, 5, normalizer="softsign"), kanode.KDense(10, 41, 5, normalizer="softsign"))
    rhs = kanode.ChainRHS(chain, device=device())
    x = np.linspace(-1.0, 1.0, 41)
    a = np.random.default_rng(4).normal(0.0, 0.1, (2, 3))
    u0 = t(-np.sin(np.pi * x)[None, :] + sum(a[:, k:k + 1] * np.sin((k + 1) * np.pi * x)[None, :] for k in range(3)))
    p0 = t(chain.setup(np.random.default_rng(0))[0].astype(np.float64))
    ts = [0.0, 0.1, 0.3, 0.5]
    w = np.random.default_rng(3).normal(size=(len(ts),) + tuple(u0.shape))
    opt = kanode.Tsit5Options(abstol=1e-9, reltol=1e-9)
    res = []
    for f, dev in ((rhs, device()), (OracleChainRHS(specs), "cpu")):
        p = p0.detach().to(dev).clone().requires_grad_(True)
        x0 = u0.detach().to(dev).clone().requires_grad_(True)
        sol = kanode.solve(f, x0, (0.0, 0.5), p, ts, opt, sensealg="interpolating_adjoint")
        g, gu = torch.autograd.grad((sol.u * torch.as_tensor(w, device=dev)).sum(), [p, x0])
        res.append((sol.u.detach().cpu(), g.cpu(), gu.cpu(), sol.stats))
    (ug, gg, gug, sg), (uc, gc, guc, sc) = res
    assert sg["naccept"] == sc["naccept"] and sg["adjoint"]["naccept"] == sc["adjoint"]["naccept"]
    # (the 41-wide sums round differently on the GPU (wave/chunk order) and the CPU (sequential):
    # 1e-15-level per RHS, carried through the steps)
    assert (ug - uc).abs().max().item() <= 1e-10 * max(1.0, uc.abs().max().item())
    # the same step sequences; the GPU and CPU sums of the 41-wide layers differ at the rounding
    # level, and this problem amplifies rounding: moving p by ONE ulp moves dp by 4.2e-8 and du0 by
    # 9.5e-8 of their largest entries on the GPU (tools/diag/burgers41_spread.py,
    # profiles/r03/parity/burgers41_spread.txt; the four- and two-launch pullbacks sit at 1.2e-8 /
    # 2.5e-8 and 2.8e-8 / 6e-8 from the CPU).  The bar is that spread: 200 reltol
    assert (gg - gc).abs().max().item() <= 200 * opt.reltol * gc.abs().max().item()
    assert (gug - guc).abs().max().item() <= 200 * opt.reltol * guc.abs().max().item()


@pytest.mark.parametrize("N,G,B", [(512, 5, 4), (512, 5, 8), (512, 5, 1)])
def test_native_surrogate_fused_pair_stages_bitwise(N, G, B):
    """KANODE_OPT_PAIR_FUSE: the native InterpolatingAdjoint of a surrogate pair holds each deferred
    stage's second launch and runs it together with the next stage's first (kd_vjp_pair_ba_kernel, the
    x̄ block forming the next λs over its own chunk, ping-pong buffers).  At the Burgers shapes the
    fusion applies (one wide-in chunking on both sides); the whole adjoint, with saveat jumps, adaptive
    error control and every gradient, is bitwise the two-launch one.  The two-launch path itself is
    pinned to the CPU oracle above (Burgers-41) and in test_gpu_surrogate.py."""
    chain = kanode.Chain(kanode.KDense(N, 10, G, normalizer="softsign"), kanode.KDense(10, N, G, normalizer="softsign"))
    rhs = kanode.ChainRHS(chain, device=device())
    x = np.linspace(-1.0, 1.0, N)
    a = np.random.default_rng(N + B).normal(0.0, 0.1, (B, 3))
    u0 = t(-np.sin(np.pi * x)[None, :] + sum(a[:, k:k + 1] * np.sin((k + 1) * np.pi * x)[None, :] for k in range(3)))
    p0 = t(chain.setup(np.random.default_rng(1))[0].astype(np.float64))
    ts = [0.0, 0.01, 0.02, 0.035, 0.05]
    w = torch.as_tensor(np.random.default_rng(2).normal(size=(len(ts),) + tuple(u0.shape)), device=device())
    out = {}
    rhs.hd.set_option("pair_persist", 0)     # the launch-per-stage adjoint (its lazy / two-launch stages)
    for fuse in (1, 0):
        with rhs.hd.options(pair_fuse=fuse):
            p = p0.detach().clone().requires_grad_(True)
            x0 = u0.detach().clone().requires_grad_(True)
            sol = kanode.solve(rhs, x0, (0.0, 0.05), p, ts, kanode.Tsit5Options(), sensealg="interpolating_adjoint")
            g, gu = torch.autograd.grad((sol.u * w).sum(), [p, x0])
            out[fuse] = (sol.u.detach(), g, gu, sol.stats)
    assert out[1][3]["adjoint"]["naccept"] == out[0][3]["adjoint"]["naccept"] >= 4
    for a_, b_ in zip(out[1][:3], out[0][:3]):
        assert torch.equal(a_, b_)


def test_native_saveat_edges():
    """saveat at t0, duplicated, between steps, on the final time and past it (dropped, as the
    Python driver never reaches it)."""
    rhs, u0, p, tspan, _ = _setup("fk26")
    ts = [0.0, 0.0, 0.123456, 1.0, 1.0, 2.0, 2.5]
    opt = kanode.Tsit5Options(abstol=1e-8, reltol=1e-8)
    nat = kanode.solve(rhs, u0, tspan, p, ts, opt)
    py = kanode.solve(rhs, u0, tspan, p, ts, dataclasses.replace(opt, native=False))
    assert nat.t == py.t == ts[:6]
    assert torch.equal(nat.u[0], u0) and torch.equal(nat.u[1], u0)
    assert (nat.u - py.u).abs().max().item() <= 1e-11


def test_dense_output_reuse_is_stateless():
    """Training reuses the dense-output storage between iterations: results equal a fresh solve."""
    rhs, u0, p0, tspan, ts = _setup("fk256")
    w = t(np.random.default_rng(1).normal(size=(len(ts),) + tuple(u0.shape)))
    opt = kanode.Tsit5Options(abstol=1e-7, reltol=1e-6)
    grads = []
    for scale in (1.0, 0.5, 1.0):       # a different problem in between (other step count)
        p = (p0 * scale).requires_grad_(True)
        sol = kanode.solve(rhs, u0, tspan, p, ts, opt, sensealg="interpolating_adjoint")
        (g,) = torch.autograd.grad((sol.u * w).sum(), [p])
        grads.append(g)
    assert torch.equal(grads[0], grads[2])


def test_native_solve_rejects_bad_arguments():
    rhs, u0, p, tspan, ts = _setup("fk26")
    lib = kanode.lib()
    o = L.SolverOptsC()
    lib.kanode_solver_options_default(C.byref(o))
    out = torch.empty((2,) + tuple(u0.shape), dtype=u0.dtype, device=u0.device)
    sv = (C.c_double * 2)(1.0, 0.5)          # descending
    h = rhs.hd._h
    st = lib.kanode_solve_tsit5(h, C.c_void_p(p.data_ptr()), C.c_void_p(u0.data_ptr()), 1, 0.0, 2.0, sv, 2,
                                C.c_void_p(out.data_ptr()), C.byref(o), None, None, None)
    assert st == L.ERR_INVALID_ARG and b"ascend" in lib.kanode_last_error(h)
    o.adaptive, o.dt = 0, 0.0               # fixed step without dt
    sv = (C.c_double * 2)(0.5, 1.0)
    st = lib.kanode_solve_tsit5(h, C.c_void_p(p.data_ptr()), C.c_void_p(u0.data_ptr()), 1, 0.0, 2.0, sv, 2,
                                C.c_void_p(out.data_ptr()), C.byref(o), None, None, None)
    assert st == L.ERR_INVALID_ARG
    lib.kanode_solver_options_default(C.byref(o))
    o.maxiters = 3
    st = lib.kanode_solve_tsit5(h, C.c_void_p(p.data_ptr()), C.c_void_p(u0.data_ptr()), 1, 0.0, 2.0, sv, 2,
                                C.c_void_p(out.data_ptr()), C.byref(o), None, None, None)
    assert st == L.ERR_INVALID_ARG and b"maxiters" in lib.kanode_last_error(h)
    torch.cuda.synchronize()


def test_fixed_step_solve_captures_into_a_hip_graph():
    """adaptive = 0 never synchronises: the whole solve (with a reused dense output) replays from a
    hipGraph and reproduces the eager result."""
    rhs, u0, p, _, _ = _setup("fk256")
    tspan, ts = (0.0, 0.05), [0.0, 0.025, 0.05]
    opt = kanode.Tsit5Options(adaptive=False, dt=5e-4).to_c()
    eager, _, dense = rhs.hd.solve_tsit5(p, u0, tspan[0], tspan[1], ts, opt, keep_dense=True)
    rhs.hd.release_dense(dense)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        out, _, dense = rhs.hd.solve_tsit5(p, u0, tspan[0], tspan[1], ts, opt, keep_dense=True)   # warm (allocates)
        rhs.hd.release_dense(dense)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            out, _, dense = rhs.hd.solve_tsit5(p, u0, tspan[0], tspan[1], ts, opt, keep_dense=True)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(eager).all()
    assert torch.equal(out, eager)
    rhs.hd.release_dense(dense)


# ---- device step control (graph mode) vs host step control -----------------------------------
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("adaptive", [True, False])
def test_device_control_matches_host_control(name, adaptive):
    """control="device" (controller in tsit5_post_kernel, the solve replayed as a hipGraph) takes the
    same steps and writes the same saveat values as the host-controlled loop."""
    rhs, u0, p, tspan, ts = _setup(name)
    dt = 0.01
    if not adaptive and name in FIXED:
        tspan, dt = FIXED[name]
        ts = [x for x in ts if x <= tspan[1]] + [tspan[1]]
    f64 = u0.dtype == torch.float64
    opt = kanode.Tsit5Options(adaptive=adaptive, dt=None if adaptive else dt, abstol=1e-8 if f64 else 1e-6,
                              reltol=1e-7 if f64 else 1e-4, graph_steps=6)
    dev = kanode.solve(rhs, u0, tspan, p, ts, dataclasses.replace(opt, control="device"))
    host = kanode.solve(rhs, u0, tspan, p, ts, dataclasses.replace(opt, control="host"))
    assert dev.stats["naccept"] == host.stats["naccept"] and dev.stats["nreject"] == host.stats["nreject"]
    scale = max(1.0, host.u.abs().max().item())
    # fixed step: identical arithmetic; adaptive: dt may differ in its last bits (device pow vs libm)
    tol = (1e-13 if f64 else 1e-6) if not adaptive else max(1e-13 if f64 else 1e-6, 1e-3 * opt.reltol)
    assert (dev.u - host.u).abs().max().item() <= tol * scale


@pytest.mark.parametrize("name", ["fk256", "fk26", "lv64"])
def test_device_control_adjoint_matches_host(name):
    """The dense output recorded by the device controller feeds the same InterpolatingAdjoint."""
    rhs, u0, p0, tspan, ts = _setup(name)
    w = t(np.random.default_rng(11).normal(size=(len(ts),) + tuple(u0.shape)))
    grads = []
    for control in ("device", "host"):
        p = p0.clone().requires_grad_(True)
        sol = kanode.solve(rhs, u0, tspan, p, ts, kanode.Tsit5Options(abstol=1e-8, reltol=1e-7, control=control),
                           sensealg="interpolating_adjoint")
        (g,) = torch.autograd.grad((sol.u * w).sum(), [p])
        grads.append((g, sol.stats))
    (gd, sd), (gh, sh) = grads
    assert sd["naccept"] == sh["naccept"]
    na, nb = sd["adjoint"]["naccept"], sh["adjoint"]["naccept"]
    # the stability-limited FK256 adjoint can flip an accept/reject on last-bit dt differences
    assert abs(na - nb) <= 0.01 * nb
    tol = 1e-12 if na == nb else 50 * 1e-7
    assert (gd - gh).abs().max().item() <= tol * gh.abs().max().item()


def test_device_control_graph_reuse_and_limits():
    """The cached graph is replayed for new parameter values (tables rebuilt inside the graph),
    grows its dense-output storage past the first capacity, and reports maxiters."""
    rhs, u0, p0, tspan, ts = _setup("fk256")
    opt = kanode.Tsit5Options(abstol=1e-7, reltol=1e-6, control="device", graph_steps=4)
    w = t(np.random.default_rng(1).normal(size=(len(ts),) + tuple(u0.shape)))
    for scale in (1.0, 0.5, 1.0):
        p = (p0 * scale).requires_grad_(True)
        sol = kanode.solve(rhs, u0, tspan, p, ts, opt, sensealg="interpolating_adjoint")
        (g,) = torch.autograd.grad((sol.u * w).sum(), [p])
        ph = (p0 * scale).requires_grad_(True)
        ref = kanode.solve(rhs, u0, tspan, ph, ts, dataclasses.replace(opt, control="host"),
                           sensealg="interpolating_adjoint")
        (gr,) = torch.autograd.grad((ref.u * w).sum(), [ph])
        assert sol.stats["naccept"] == ref.stats["naccept"] and sol.stats["naccept"] > 64   # past one capacity
        assert (sol.u - ref.u).abs().max().item() <= 1e-3 * opt.reltol
        assert (g - gr).abs().max().item() <= 50 * opt.reltol * gr.abs().max().item()
    with pytest.raises(kanode.KanodeError, match="maxiters"):
        kanode.solve(rhs, u0, tspan, p0, ts, dataclasses.replace(opt, maxiters=10))


# ---- one-workgroup solve of a small chain (kd_chain_tsit5_kernel) vs the host loop ------------
def _lv_u0(B, seed=4):
    return np.random.default_rng(seed).uniform(0.5, 2.0, (B, 2))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("adaptive", [True, False])
def test_fused_chain_solve_matches_host_loop(dtype, B, adaptive):
    """control="auto" runs a <= 16-trajectory small chain as ONE workgroup (controller, saveat and
    dense output on the device); it takes the host loop's steps and writes the same saveat values,
    and its dense output feeds the same InterpolatingAdjoint."""
    rhs = lv(dtype)
    u0 = t(_lv_u0(B), dtype)
    p0 = t(np.random.default_rng(7).uniform(-0.3, 0.3, 240), dtype)
    tspan, ts = (0.0, 3.5), [0.1 * i for i in range(35)]
    f64 = dtype == torch.float64
    opt = kanode.Tsit5Options(adaptive=adaptive, dt=None if adaptive else 0.01, abstol=1e-8 if f64 else 1e-6,
                              reltol=1e-7 if f64 else 1e-4)
    w = t(np.random.default_rng(11).normal(size=(len(ts), B, 2)), dtype)
    out = {}
    for control in ("auto", "host"):
        p = p0.clone().requires_grad_(True)
        sol = kanode.solve(rhs, u0, tspan, p, ts, dataclasses.replace(opt, control=control),
                           sensealg="interpolating_adjoint")
        (g,) = torch.autograd.grad((sol.u * w).sum(), [p])
        out[control] = (sol, g)
    (sf, gf), (sh, gh) = out["auto"], out["host"]
    # adaptive: the error norm is one block sum (host: slab partials) and pow() runs on the device,
    # so dt may differ in its last bits; fp32 adaptive may then flip a step decision
    if f64 or not adaptive:
        assert sf.stats["naccept"] == sh.stats["naccept"] and sf.stats["nreject"] == sh.stats["nreject"]
        assert sf.stats["nf"] == sh.stats["nf"]
    else:
        assert abs(sf.stats["naccept"] - sh.stats["naccept"]) <= 2
    scale = max(1.0, sh.u.abs().max().item())
    tol = (1e-12 if f64 else 2e-6) if not adaptive else max(1e-12 if f64 else 2e-6, 1e-3 * opt.reltol)
    if not f64 and adaptive:
        tol = 20 * opt.reltol
    assert (sf.u - sh.u).abs().max().item() <= tol * scale
    gtol = 1e-9 if f64 else 5e-3
    assert (gf - gh).abs().max().item() <= gtol * gh.abs().max().item()


@pytest.mark.parametrize("ts", [[0.0, 0.5, 0.5, 1.2, 3.5], [0.25, 3.0], [3.5]])
def test_fused_chain_adjoint_saveat_edges(ts):
    """The one-workgroup adjoint's jumps: saveat at t0 (applied after the loop), duplicates (rows
    summed), tf (the initial λ) and interior stops, against the host loop."""
    rhs = lv()
    u0 = t(_lv_u0(3, 6))
    p0 = t(np.random.default_rng(8).uniform(-0.3, 0.3, 240))
    opt = kanode.Tsit5Options(abstol=1e-8, reltol=1e-7)
    w = t(np.random.default_rng(3).normal(size=(len(ts), 3, 2)))
    res = {}
    for control in ("auto", "host"):
        p = p0.clone().requires_grad_(True)
        u = u0.clone().requires_grad_(True)
        sol = kanode.solve(rhs, u, (0.0, 3.5), p, ts, dataclasses.replace(opt, control=control),
                           sensealg="interpolating_adjoint")
        gp, gu = torch.autograd.grad((sol.u * w).sum(), [p, u])
        res[control] = (sol, gp, gu)
    (sa, pa, ua), (sh, ph, uh) = res["auto"], res["host"]
    assert sa.stats["adjoint"]["naccept"] == sh.stats["adjoint"]["naccept"]
    assert (pa - ph).abs().max().item() <= 1e-9 * ph.abs().max().item()
    assert (ua - uh).abs().max().item() <= 1e-9 * max(1e-300, uh.abs().max().item())


def test_fused_chain_repeated_calls_with_changing_saveat_are_bitwise_fresh():
    """Round 6: the one-workgroup solve and adjoint skip a saveat / stop upload whose bytes equal the last one, and
    read their counters and step records from mapped host memory (kanode_solve.cpp solve_fused_t, adjoint_fused_t).
    Alternating saveat lists (same length, other values; another length; back) on ONE handle, with and without
    a gradient, give bitwise what a fresh handle gives, step records included."""
    u0 = t(_lv_u0(2, 9))
    p0 = t(np.random.default_rng(12).uniform(-0.3, 0.3, 240))
    opt = kanode.Tsit5Options(abstol=1e-8, reltol=1e-7)
    lists = [[0.1 * i for i in range(35)], [0.1 * i + 0.05 for i in range(35)], [0.0, 1.0, 3.5],
             [0.1 * i for i in range(35)], [0.0, 1.0, 3.5]]

    def run(rhs, ts, grad):
        w = t(np.random.default_rng(len(ts)).normal(size=(len(ts), 2, 2)))
        p = p0.clone().requires_grad_(grad)
        sol = kanode.solve(rhs, u0, (0.0, 3.5), p, ts, opt, sensealg="interpolating_adjoint")
        if not grad:
            return sol.u.detach().cpu(), None, sol.stats["naccept"], None
        (g,) = torch.autograd.grad((sol.u * w).sum(), [p])
        return sol.u.detach().cpu(), g.cpu(), sol.stats["naccept"], sol.stats.get("dts")

    shared = lv()
    for grad in (False, True):
        for ts in lists:
            got, want = run(shared, ts, grad), run(lv(), ts, grad)
            assert torch.equal(got[0], want[0]) and got[2] == want[2]
            if grad:
                assert torch.equal(got[1], want[1]) and got[3] == want[3]


def test_fused_chain_solve_falls_back_when_dense_output_fills():
    """A dense output larger than the fused block (KANODE_OPT_FUSED_SOLVE_CAP) falls back to the
    host loop: same steps, same values, a usable dense output."""
    rhs = lv()
    u0 = t(_lv_u0(2))
    p0 = t(np.random.default_rng(7).uniform(-0.3, 0.3, 240))
    ts = [0.1 * i for i in range(35)]
    opt = kanode.Tsit5Options(abstol=1e-8, reltol=1e-7)
    w = t(np.random.default_rng(2).normal(size=(len(ts), 2, 2)))
    ref_p = p0.clone().requires_grad_(True)
    ref = kanode.solve(rhs, u0, (0.0, 3.5), ref_p, ts, dataclasses.replace(opt, control="host"),
                       sensealg="interpolating_adjoint")
    (gr,) = torch.autograd.grad((ref.u * w).sum(), [ref_p])
    p = p0.clone().requires_grad_(True)
    with rhs.hd.options(fused_solve_cap=3):
        sol = kanode.solve(rhs, u0, (0.0, 3.5), p, ts, opt, sensealg="interpolating_adjoint")
        (g,) = torch.autograd.grad((sol.u * w).sum(), [p])
    assert sol.stats["naccept"] == ref.stats["naccept"] > 3
    assert (sol.u - ref.u).abs().max().item() <= 1e-12 * max(1.0, ref.u.abs().max().item())
    assert (g - gr).abs().max().item() <= 1e-12 * gr.abs().max().item()


def _fk_cfg(nx, G, norm, basis="rbf"):
    kan1 = kanode.Chain(kanode.KDense(1, 1, G, normalizer=norm, basis_func=basis))
    return kanode.FisherKPPRHS(kan1, nx=nx, dx=1.0 / (nx - 1), D=0.01, device=device())


def _fused_vs_staged(rhs, u0, p0, tspan, ts, opt, grids=None):
    """Solve + InterpolatingAdjoint with the one-launch step kernels (KANODE_OPT_FUSED_STEP = 1) and
    with per-stage launches (0); returns ((sol, dp, du0) fused, (sol, dp, du0) staged)."""
    w = t(np.random.default_rng(12).normal(size=(len(ts),) + tuple(u0.shape)))
    out = {}
    for fused in (1, 0):
        # (both on the host loop: the step kernels' arithmetic is compared, not the device step control,
        # whose controller rounds differently -- test_fk_device_loop_matches_host_loop)
        with rhs.hd.options(fused_step=fused, fk_device_loop=0, **(grids or {})):
            p = p0.clone().requires_grad_(True)
            x0 = u0.clone().requires_grad_(True)
            sol = kanode.solve(rhs, x0, tspan, p, ts, opt, sensealg="interpolating_adjoint")
            g, gu = torch.autograd.grad((sol.u * w).sum(), [p, x0])
        out[fused] = (sol, g, gu)
    return out[1], out[0]


def _check_fused_vs_staged(fused, staged, adaptive):
    (sf, gf, guf), (ss, gs, gus) = fused, staged
    assert sf.stats["naccept"] == ss.stats["naccept"] and sf.stats["nreject"] == ss.stats["nreject"]
    assert abs(sf.stats["adjoint"]["naccept"] - ss.stats["adjoint"]["naccept"]) <= (1 if adaptive else 0)
    scale = max(1.0, ss.u.abs().max().item())
    assert (sf.u - ss.u).abs().max().item() <= 1e-12 * scale
    assert (gf - gs).abs().max().item() <= 1e-9 * gs.abs().max().item()
    assert (guf - gus).abs().max().item() <= 1e-9 * gus.abs().max().item()


@pytest.mark.parametrize("adaptive", [True, False])
@pytest.mark.parametrize("nx", [128, 256, 512])
@pytest.mark.parametrize("G,norm", [(10, "softsign"), (5, "tanh_fast")])
def test_fused_fk_step_matches_stage_launches(adaptive, nx, G, norm):
    """The one-launch Tsit5 step (fk_step_pp_wave_kernel, Q-form dense output) and adjoint step
    (fk_vjp_step_pp_wave_kernel) against the per-stage launches with the K-form dense output
    (KANODE_OPT_FUSED_STEP = 0): same steps, saveat values, dL/dp and dL/du0.  Nx = 128/256/512 are
    the NP = 1/2/4 instantiations (the periodic wrap crosses pairs for NP > 1)."""
    rhs = _fk_cfg(nx, G, norm)
    u0 = t(fk_u0(nx, 4))
    p0 = t(np.random.default_rng(7).uniform(-1.0, 1.0, G + 1))
    # D lap has eigenvalues down to -4 D / dx^2 (-2611 at Nx = 512): the fixed step is scaled to stay
    # inside Tsit5's stability region, and the adaptive tolerance is tight enough that accuracy, not
    # stability, picks the steps (at the stability edge rounding differences are amplified: 1e-9
    # relative in du0 at reltol 1e-7, Nx = 512; tools/diag/fused_np4.py)
    if adaptive:
        tspan, ts = (0.0, 1.0), [0.25 * i for i in range(5)]
    else:
        tspan, ts = (0.0, 0.1), [0.0, 0.05, 0.1]
    dt = 5e-4 * (256 / nx) ** 2
    opt = kanode.Tsit5Options(adaptive=adaptive, dt=None if adaptive else dt, abstol=1e-11, reltol=1e-10)
    _check_fused_vs_staged(*_fused_vs_staged(rhs, u0, p0, tspan, ts, opt), adaptive)


@pytest.mark.parametrize("nx", [128, 256, 512])
def test_fused_fk_step_several_rows_per_wave(nx):
    """Persistent grids of ONE block (KANODE_OPT_GRID_*=1): each of its 4 waves runs 3 trajectory rows
    through the forward step, the adjoint step and the per-stage kernels, so the row loops, the
    per-row register reuse and the block-level moment sums over several rows are exercised."""
    rhs = _fk_cfg(nx, 10, "softsign")
    u0 = t(fk_u0(nx, 12, 3))
    p0 = t(np.random.default_rng(8).uniform(-1.0, 1.0, 11))
    opt = kanode.Tsit5Options(abstol=1e-11, reltol=1e-10)
    ts = [0.0, 0.2, 0.5]
    one = dict(grid_rhs=1, grid_vjp=1, grid_adj_step=1)
    fused, staged = _fused_vs_staged(rhs, u0, p0, (0.0, 0.5), ts, opt, one)
    _check_fused_vs_staged(fused, staged, True)
    # the single-block grid against the default grid at a fixed step: the solution is bitwise equal
    # (only reduction orders differ: dp, and in adaptive runs the error norm and so the step sizes)
    fixed = kanode.Tsit5Options(adaptive=False, dt=5e-4 * (256 / nx) ** 2)
    (s1, g1, gu1), _ = _fused_vs_staged(rhs, u0, p0, (0.0, 0.1), [0.0, 0.05, 0.1], fixed, one)
    (sd, gd, gud), _ = _fused_vs_staged(rhs, u0, p0, (0.0, 0.1), [0.0, 0.05, 0.1], fixed)
    assert torch.equal(s1.u, sd.u)
    assert (g1 - gd).abs().max().item() <= 1e-12 * gd.abs().max().item()
    assert (gu1 - gud).abs().max().item() <= 1e-13 * gud.abs().max().item()


def _solve_grad(rhs, u0, p0, tspan, ts, opt, **opts):
    w = t(np.random.default_rng(13).normal(size=(len(ts),) + tuple(u0.shape)))
    with rhs.hd.options(**opts):
        p = p0.clone().requires_grad_(True)
        x0 = u0.clone().requires_grad_(True)
        sol = kanode.solve(rhs, x0, tspan, p, ts, opt, sensealg="interpolating_adjoint")
        g, gu = torch.autograd.grad((sol.u * w).sum(), [p, x0])
    return sol, g, gu


@pytest.mark.parametrize("adaptive", [True, False])
@pytest.mark.parametrize("nx,B", [(128, 6), (256, 6), (256, 37)])
def test_adjoint_step_rows_kernel_matches_persistent_grid(nx, B, adaptive):
    """The adjoint step with one row per wave and the row's stage values in registers
    (fk_vjp_step_rows_kernel, the default up to 8192 rows of <= 256 points) against the
    persistent-grid step kernel that passes kλ through memory (KANODE_OPT_ADJ_STEP_ROWS = 0).
    B = 6 and 37 leave idle waves in the last block.  At a fixed step λ (dL/du0) is bitwise equal
    (the stage arithmetic is the same, statement for statement) and dL/dp equal to the reduction
    order.  Adaptive runs put adjoint stages in other forward steps than their step's first stage
    (the dense-output reload) and take their step sizes from the [λ; μ] error norm."""
    rhs = _fk_cfg(nx, 10, "softsign")
    u0 = t(fk_u0(nx, B, 5))
    p0 = t(np.random.default_rng(11).uniform(-1.0, 1.0, 11))
    if adaptive:   # tolerances at which accuracy, not the stability limit, picks the steps (see above)
        tspan, ts, opt = (0.0, 0.5), [0.0, 0.2, 0.45, 0.5], kanode.Tsit5Options(abstol=1e-11, reltol=1e-10)
    else:
        tspan, ts = (0.0, 0.1), [0.0, 0.05, 0.1]
        opt = kanode.Tsit5Options(adaptive=False, dt=5e-4 * (256 / nx) ** 2)
    # (both on the host step control: the kernels are compared, test_fk_device_loop_matches_host_loop covers
    # the device loops)
    s1, g1, gu1 = _solve_grad(rhs, u0, p0, tspan, ts, opt, fk_device_loop=0)
    s0, g0, gu0 = _solve_grad(rhs, u0, p0, tspan, ts, opt, adj_step_rows=0, fk_device_loop=0)
    assert torch.equal(s1.u, s0.u)
    if adaptive:
        # μ starts at 0, so its error scale is abstol and the μ error estimate (a difference of
        # reduced sums) carries the reductions' rounding: the two kernels' step sequences can part
        # on last-bit differences (as in test_native_adjoint_matches_python_adjoint); both then
        # solve the same adjoint to the tolerance.  The persistent-grid kernel's grid (and so its
        # reduction order) follows its occupancy, so which step sequence it takes moves with its
        # register count; measured: up to 6.7e-9 of max|dL/du0| (67·reltol) with different step
        # counts (round 4), 1e-9 with equal ones.  The fixed-step cases below are the arithmetic check
        na, nb = s1.stats["adjoint"]["naccept"], s0.stats["adjoint"]["naccept"]
        assert abs(na - nb) <= 0.01 * nb
        tol = 1e-9 if na == nb else 200 * opt.reltol
        assert (g1 - g0).abs().max().item() <= tol * g0.abs().max().item()
        assert (gu1 - gu0).abs().max().item() <= tol * gu0.abs().max().item()
    else:
        assert s1.stats["adjoint"]["naccept"] == s0.stats["adjoint"]["naccept"]
        assert (g1 - g0).abs().max().item() <= 1e-12 * g0.abs().max().item()
        assert torch.equal(gu1, gu0)


@pytest.mark.parametrize("nx,B", [(256, 45), (256, 512), (128, 4096)])
def test_adjoint_fused_finish_bitwise(nx, B):
    """KANODE_OPT_ADJ_FUSED_FINISH = 1: the adaptive rows step finishes inside its own launch (the last 1 + P
    workgroups to arrive each run one block of adj_finish_kernel, in its order) instead of the separate finish
    launch (the default): the same step sequence, and solution and gradients bitwise equal.  B = 45 is the
    smallest batch with the 12 workgroups it needs (P = 11); smaller batches take the finish launch."""
    rhs = _fk_cfg(nx, 10, "softsign")
    u0 = t(fk_u0(nx, B, 8))
    p0 = t(np.random.default_rng(21).uniform(-1.0, 1.0, 11))
    opt = kanode.Tsit5Options(abstol=1e-9, reltol=1e-8)
    tspan, ts = (0.0, 0.3), [0.0, 0.1, 0.25, 0.3]
    assert rhs.hd.get_option("adj_fused_finish") == 0
    # (on the host step control, which the fused finish runs under)
    s1, g1, gu1 = _solve_grad(rhs, u0, p0, tspan, ts, opt, adj_fused_finish=1, fk_device_loop=0)
    s0, g0, gu0 = _solve_grad(rhs, u0, p0, tspan, ts, opt, fk_device_loop=0)
    assert s1.stats["adjoint"] == s0.stats["adjoint"]
    assert torch.equal(s1.u, s0.u) and torch.equal(g1, g0) and torch.equal(gu1, gu0)
    # and again on the same handle (the arrival counters are back at zero after every step)
    s2, g2, gu2 = _solve_grad(rhs, u0, p0, tspan, ts, opt, adj_fused_finish=1, fk_device_loop=0)
    assert torch.equal(g2, g1) and torch.equal(gu2, gu1)


@pytest.mark.parametrize("nx,B", [(256, 64), (128, 300), (512, 5)])
def test_fk_device_loop_matches_host_loop(nx, B):
    """KANODE_OPT_FK_DEVICE_LOOP (the default for an adaptive table-path solve that keeps its dense output):
    every step launch reads its step size from device memory and the launch's last workgroup runs the PI
    controller, the host queues 16-launch batches ahead and the saveat values come from the dense output
    afterwards.  Against the host loop (FK_DEVICE_LOOP = 0, one norm read per step): the device sums the
    error partials in another order and its pow may round the last bit differently, so the step sizes part
    at the rounding level, and where the stability limit rather than accuracy sets the steps the PI
    controller amplifies that (measured on a stability-limited FK128 run: 4e-5 after 1,300 steps, the
    solution 0.3·reltol apart).  Bars: step counts within 1%, steps to 1e-3, the solution to 10·reltol and
    the gradients to 100·reltol of their scale; the device loop itself bitwise reproducible.  The saveat
    points fall inside steps, on step ends and at t0; the solve ends mid-batch (the launches queued behind
    return at once); two solves on one handle (the arrival counter is back at zero); maxiters ends the
    device loop with the host loop's error."""
    rhs = _fk_cfg(nx, 10, "softsign")
    u0 = t(fk_u0(nx, B, 4))
    p0 = t(np.random.default_rng(9).uniform(-1.0, 1.0, 11))
    opt = kanode.Tsit5Options(abstol=1e-9, reltol=1e-8)
    tspan, ts = (0.0, 0.4), [0.0, 0.1, 0.25, 0.3, 0.4]
    assert rhs.hd.get_option("fk_device_loop") == 1
    rhs.hd.set_option("record_adjoint_steps", 1)
    sd, gd, gud = _solve_grad(rhs, u0, p0, tspan, ts, opt)
    sd2, gd2, gud2 = _solve_grad(rhs, u0, p0, tspan, ts, opt)
    sh, gh, guh = _solve_grad(rhs, u0, p0, tspan, ts, opt, fk_device_loop=0)
    for st in (sd.stats, sh.stats):   # the backward steps (the device loop's records) tile the span
        hs = np.asarray(st["adjoint"]["dts"])
        assert len(hs) == st["adjoint"]["naccept"] and abs(hs.sum() - 0.4) <= 1e-12
    assert sd.stats["adjoint"] == sd2.stats["adjoint"]
    ad, ah = sd.stats["adjoint"]["naccept"], sh.stats["adjoint"]["naccept"]
    assert abs(ad - ah) <= 0.01 * ah
    assert torch.equal(sd.u, sd2.u) and torch.equal(gd, gd2) and torch.equal(gud, gud2)
    na, nh = sd.stats["naccept"], sh.stats["naccept"]
    assert abs(na - nh) <= 0.01 * nh and na > 16
    print(f"steps {na}/{nh}, rejects {sd.stats['nreject']}/{sh.stats['nreject']}, adjoint steps {ad}/{ah}")
    if na == nh:
        dd = np.abs(np.divide(sd.stats["dts"], sh.stats["dts"]) - 1).max()
        print(f"max step difference {dd:.2e}")
        assert dd <= 1e-3
    assert (sd.u - sh.u).abs().max().item() <= 10 * opt.reltol * sh.u.abs().max().item()
    for a_, b_ in ((gd, gh), (gud, guh)):
        assert (a_ - b_).abs().max().item() <= 100 * opt.reltol * b_.abs().max().item()
    # the native forward alone (no gradient, no dense output kept: the host loop)
    with torch.no_grad():
        nd = kanode.solve(rhs, u0, tspan, p0, ts, opt)
    assert (nd.u - sh.u).abs().max().item() <= 1e-12 * sh.u.abs().max().item()
    with pytest.raises(RuntimeError, match="maxiters"):
        _solve_grad(rhs, u0, p0, tspan, ts, dataclasses.replace(opt, maxiters=5))


def test_adjoint_step_rows_kernel_batch_cap():
    """Above 8192 rows (one row per wave: 4 rows x the 2048 slab blocks) the adjoint step falls back
    to the persistent-grid kernel: both settings of KANODE_OPT_ADJ_STEP_ROWS then run the same
    kernel."""
    rhs = _fk_cfg(128, 10, "softsign")
    u0 = t(np.tile(fk_u0(128, 16, 6), (513, 1)))    # 8208 rows
    p0 = t(np.random.default_rng(12).uniform(-1.0, 1.0, 11))
    opt = kanode.Tsit5Options(adaptive=False, dt=2e-3)
    s1, g1, gu1 = _solve_grad(rhs, u0, p0, (0.0, 0.006), [0.0, 0.006], opt)
    s0, g0, gu0 = _solve_grad(rhs, u0, p0, (0.0, 0.006), [0.0, 0.006], opt, adj_step_rows=0)
    assert torch.equal(s1.u, s0.u) and torch.equal(g1, g0) and torch.equal(gu1, gu0)


@pytest.mark.parametrize("norm,basis", [("sigmoid", "rbf"), ("softsign", "rswaf")])
def test_qform_forward_with_per_stage_adjoint(norm, basis):
    """Table-path configurations the fused adjoint step does not cover (fk_vjp_pp_supported false:
    sigmoid normalizer, rswaf basis): the forward runs the one-launch step with the Q-form dense
    output and the adjoint feeds the 4-array Q-form interpolant into the per-stage VJP.  Checked
    against the all-per-stage run (K-form dense output) on dL/dp and dL/du0."""
    rhs = _fk_cfg(256, 10, norm, basis)
    assert rhs.hd.pointwise_table
    u0 = t(fk_u0(256, 3, 4))
    p0 = t(np.random.default_rng(9).uniform(-1.0, 1.0, 11))
    opt = kanode.Tsit5Options(abstol=1e-11, reltol=1e-10)
    _check_fused_vs_staged(*_fused_vs_staged(rhs, u0, p0, (0.0, 0.5), [0.0, 0.25, 0.5], opt), True)


def test_options_round_trip_and_reject_bad_values():
    rhs = fk(256)
    hd = rhs.hd
    assert hd.get_option("fused_step") == 1 and hd.get_option("fused_solve") == 1
    assert hd.get_option("grid_rhs") == hd.get_option("grid_vjp") == hd.get_option("grid_adj_step") == 0
    assert hd.get_option("adj_step_rows") == 1 and hd.get_option("adj_fused_finish") == 0
    with hd.options(fused_step=0, grid_vjp=7):
        assert hd.get_option("fused_step") == 0 and hd.get_option("grid_vjp") == 7
    assert hd.get_option("fused_step") == 1 and hd.get_option("grid_vjp") == 0
    for name, bad in (("fused_step", 2), ("grid_rhs", -1), ("grid_vjp", 1 << 20), ("fused_solve_cap", -3)):
        with pytest.raises(L.KanodeError):
            hd.set_option(name, bad)
    with pytest.raises(KeyError):
        hd.set_option("no_such_option", 1)


def test_failed_adjoint_leaves_no_pending_stage():
    """a lazy surrogate-pair adjoint stage keeps raw pointers into the solution and the
    handle's workspace until the next stage.  An adjoint that fails mid-run (here: maxiters) must drop it:
    afterwards the same handle's adjoint stage and a full adjoint over the same dense output equal a fresh
    handle's, bit for bit (a stale second launch would have added into them)."""
    N, G, B = 512, 5, 4
    mk = lambda: kanode.ChainRHS(kanode.Chain(kanode.KDense(N, 10, G, normalizer="softsign"),   # noqa: E731
                                              kanode.KDense(10, N, G, normalizer="softsign")), device=device())
    rhs, fresh = mk(), mk()
    x = np.linspace(-1.0, 1.0, N)
    a = np.random.default_rng(7).normal(0.0, 0.1, (B, 3))
    u0 = t(-np.sin(np.pi * x)[None, :] + sum(a[:, k:k + 1] * np.sin((k + 1) * np.pi * x)[None, :] for k in range(3)))
    p = t(rhs.chain.setup(np.random.default_rng(1))[0].astype(np.float64))
    ts = [0.0, 0.01, 0.02, 0.035, 0.05]
    g = torch.as_tensor(np.random.default_rng(2).normal(size=(len(ts),) + tuple(u0.shape)), device=device())
    opt = kanode.Tsit5Options()
    for r in (rhs, fresh):
        r.hd.set_option("pair_fuse", 1)
        r.hd.set_option("pair_persist", 0)   # the launch-per-stage adjoint, whose lazy stages this is about
    _, _, dense = rhs.hd.solve_tsit5(p, u0, 0.0, 0.05, ts, opt.to_c(), keep_dense=True)
    bad = opt.to_c()
    bad.maxiters = 2
    with pytest.raises(kanode.KanodeError, match="maxiters"):
        rhs.hd.adjoint_tsit5(p, dense, g, bad, tuple(u0.shape))
    lam = torch.as_tensor(np.random.default_rng(3).normal(size=tuple(u0.shape)), device=device())
    r1 = rhs.hd.vjp_stage(p, u0, [], [], lam, [], [])
    r2 = fresh.hd.vjp_stage(p, u0, [], [], lam, [], [])
    torch.cuda.synchronize()
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])
    du0, dp, st = rhs.hd.adjoint_tsit5(p, dense, g, opt.to_c(), tuple(u0.shape))
    _, _, dense2 = fresh.hd.solve_tsit5(p, u0, 0.0, 0.05, ts, opt.to_c(), keep_dense=True)
    du0f, dpf, stf = fresh.hd.adjoint_tsit5(p, dense2, g, opt.to_c(), tuple(u0.shape))
    assert st == stf
    assert torch.equal(du0, du0f) and torch.equal(dp, dpf)


def _surrogate_ics(name, N, B, seed):
    rng = np.random.default_rng(seed)
    if name == "burgers512":
        x = np.linspace(-1.0, 1.0, N)
        a = rng.normal(0.0, 0.1, (B, 3))
        return -np.sin(np.pi * x)[None, :] + sum(a[:, k:k + 1] * np.sin((k + 1) * np.pi * x)[None, :] for k in range(3))
    x = np.linspace(-5.0, 5.0, N // 2)
    amp, th = rng.uniform(0.8, 1.2, (B, 1)), rng.uniform(0.0, 2 * np.pi, (B, 1))
    env = amp * 2.0 / np.cosh(x)[None, :]
    return np.concatenate([env * np.cos(th), env * np.sin(th)], axis=1)


@pytest.mark.parametrize("name,N,G,B,persist", [("burgers512", 512, 5, 4, 1), ("burgers512", 512, 5, 4, 0),
                                                ("schrodinger1024", 2048, 10, 8, 1)])
@pytest.mark.parametrize("adaptive", [False, True])
def test_full_size_surrogate_adjoint_matches_cpu_oracle(name, N, G, B, persist, adaptive):
    """the BASELINE configs[3]/[4] surrogates at their bench sizes (Burgers KAN [512, 10, 512]
    G=5, 4 ICs; Schrödinger KAN [2048, 10, 2048] G=10, 8 ICs; Burgers_Surrogate.jl:85-107,187-206,
    Schrodinger_Surrogate.jl:93-104,198-217), native solve + InterpolatingAdjoint against the Python driver over
    the C oracle chain: at the Burgers shape both the one-launch adjoint (kd_pair_adjoint_kernel, the default)
    and the launch-per-stage one (fused kd_vjp_pair_ba_kernel stages); Schrödinger's LDS carve does not fit
    the one-launch kernel, so it runs per stage either way.

    Bars.  Fixed steps (same step sequence by construction): every RHS / VJP the GPU evaluates is within
    1e-13 of its Σ|terms| scale of the oracle's (test_gpu_surrogate.py); the solution is a sum of
    ~6·n_steps such evaluations times h, and dp = μ(t0) a sum of ~6·n_adjoint_steps stage VJPs times h, so
    both stay within n_evals·1e-13 of their scale over this short span (T·Lipschitz < 1, no growth), i.e.
    1e-13 × the evaluation count: 1.2e-11 for the solution (120 RHS) and 2.6e-11 for the gradients here.
    Adaptive: the controllers see the embedded error estimate, a difference of nearly equal terms, so the
    stage values' 1e-13 differences move each step by a relative δ (measured from both step sequences,
    forward and adjoint: kanode_solution_step_sizes / KANODE_OPT_RECORD_ADJOINT_STEPS against the driver's;
    the PI controller carries them from step to step: up to 2.3e-5 measured, the Schrödinger adjoint).
    VERDICT r4 #4: instead of a widened bar, the oracle then REPLAYS the GPU's accepted step sequences
    (Tsit5Options.replay_dts / replay_adjoint_dts), so the GPU's arithmetic is checked at the fixed-step bars
    on the same grid; separately, on its own grid the oracle takes the same step counts, steps within 1e-3
    (a controller that diverged while keeping the count moves them by percents) and results within
    10·reltol."""
    from oracle_rhs import OracleChainRHS
    specs = [O.LayerSpec(N, 10, G, "softsign"), O.LayerSpec(10, N, G, "softsign")]
    chain = kanode.Chain(kanode.KDense(N, 10, G, normalizer="softsign"), kanode.KDense(10, N, G, normalizer="softsign"))
    rhs = kanode.ChainRHS(chain, device=device())
    rhs.hd.set_option("pair_persist", persist)   # 1: the one-launch adjoint where it fits (Burgers), else per stage
    rhs.hd.set_option("record_adjoint_steps", 1)
    u0 = t(_surrogate_ics(name, N, B, 11))
    p0 = t(chain.setup(np.random.default_rng(0))[0].astype(np.float64))
    T = 0.05
    ts = [0.0, 0.02, 0.035, 0.05]
    w = np.random.default_rng(3).normal(size=(len(ts),) + tuple(u0.shape))
    opt = kanode.Tsit5Options(abstol=1e-8, reltol=1e-8) if adaptive else kanode.Tsit5Options(adaptive=False, dt=0.0025)
    res = []
    for f, dev, o in ((rhs, device(), opt), (OracleChainRHS(specs), "cpu", opt)):
        p = p0.detach().to(dev).clone().requires_grad_(True)
        x0 = u0.detach().to(dev).clone().requires_grad_(True)
        sol = kanode.solve(f, x0, (0.0, T), p, ts, o, sensealg="interpolating_adjoint")
        g, gu = torch.autograd.grad((sol.u * torch.as_tensor(w, device=dev)).sum(), [p, x0])
        res.append((sol.u.detach().cpu(), g.cpu(), gu.cpu(), sol.stats))
    (ug, gg, gug, sg), (uc, gc, guc, sc) = res
    assert sg["naccept"] == sc["naccept"] and sg["adjoint"]["naccept"] == sc["adjoint"]["naccept"]
    assert len(sg["dts"]) == sg["naccept"] and len(sg["adjoint"]["dts"]) == sg["adjoint"]["naccept"]
    d_f = float(np.max(np.abs(np.divide(sg["dts"], sc["dts"]) - 1.0)))
    d_a = float(np.max(np.abs(np.divide(sg["adjoint"]["dts"], sc["adjoint"]["dts"]) - 1.0)))
    rel = lambda a_, b_: (a_ - b_).abs().max().item() / b_.abs().max().item()   # noqa: E731
    if adaptive:
        assert d_f <= 1e-3 and d_a <= 1e-3, (d_f, d_a)
        assert rel(ug, uc) <= 10 * opt.reltol and max(rel(gg, gc), rel(gug, guc)) <= 10 * opt.reltol
        own = f"own grid: u {rel(ug, uc):.1e}, dp {rel(gg, gc):.1e}; "
        # the oracle on the GPU's grid
        rep = dataclasses.replace(opt, adaptive=False, replay_dts=tuple(sg["dts"]),
                                  replay_adjoint_dts=tuple(sg["adjoint"]["dts"]))
        p = p0.detach().cpu().clone().requires_grad_(True)
        x0 = u0.detach().cpu().clone().requires_grad_(True)
        sol = kanode.solve(OracleChainRHS(specs), x0, (0.0, T), p, ts, rep, sensealg="interpolating_adjoint")
        gc, guc = torch.autograd.grad((sol.u * torch.as_tensor(w)).sum(), [p, x0])
        uc, sc = sol.u.detach(), sol.stats
        assert sc["naccept"] == sg["naccept"] and sc["adjoint"]["naccept"] == sg["adjoint"]["naccept"]
        assert np.array_equal(sc["dts"], sg["dts"]) and np.array_equal(sc["adjoint"]["dts"], sg["adjoint"]["dts"])
    else:
        assert d_f <= 1e-12 and d_a <= 1e-12, (d_f, d_a)
        own = ""
    bar_u = 1e-13 * sc["nf"]
    bar_g = 1e-13 * sc["adjoint"]["nf"]
    eu, eg, egu = rel(ug, uc), rel(gg, gc), rel(gug, guc)
    print(f"{name} adaptive={adaptive}: steps {sg['naccept']}/{sg['adjoint']['naccept']} (step perturbation "
          f"{d_f:.1e} / {d_a:.1e}), {own}same grid: rel err u {eu:.2e} "
          f"(bar {bar_u:.1e}), dp {eg:.2e}, du0 {egu:.2e} (bar {bar_g:.1e})")
    assert eu <= bar_u
    assert eg <= bar_g and egu <= bar_g


@pytest.mark.parametrize("N,G,B,S", [(512, 5, 4, 0), (512, 5, 1, 0), (41, 5, 2, 0), (512, 5, 4, 4), (41, 5, 3, 4)])
@pytest.mark.parametrize("adaptive", [True, False])
def test_persistent_pair_adjoint_matches_launch_path(N, G, B, S, adaptive):
    """KANODE_OPT_PAIR_PERSIST: the whole surrogate adjoint as one launch (kd_pair_adjoint_kernel: the grid
    split over workgroups of S points, two exchanges of the hidden partials per stage, μ in LDS, the step
    control on the device) against the launch-per-stage native adjoint, which the full-size oracle test
    above pins.  Same algorithm, sums in another fixed order: equal step counts, gradients to 1e-11 of
    their scale (fixed steps) / 1e-9 (adaptive: the step sizes move with the rounding of the error norm);
    bitwise reproducible between two runs.  KANODE_OPT_LAST_ADJOINT shows which path ran (a
    shape the kernel rejects would otherwise compare the launch path with itself)."""
    chain = kanode.Chain(kanode.KDense(N, 10, G, normalizer="softsign"), kanode.KDense(10, N, G, normalizer="softsign"))
    rhs = kanode.ChainRHS(chain, device=device())
    x = np.linspace(-1.0, 1.0, N)
    a = np.random.default_rng(N + B).normal(0.0, 0.1, (B, 3))
    u0 = t(-np.sin(np.pi * x)[None, :] + sum(a[:, k:k + 1] * np.sin((k + 1) * np.pi * x)[None, :] for k in range(3)))
    p0 = t(chain.setup(np.random.default_rng(1))[0].astype(np.float64))
    ts = [0.0, 0.01, 0.02, 0.035, 0.05]
    w = torch.as_tensor(np.random.default_rng(2).normal(size=(len(ts),) + tuple(u0.shape)), device=device())
    opt = kanode.Tsit5Options() if adaptive else kanode.Tsit5Options(adaptive=False, dt=0.004)
    out = []
    for persist in (1, 1, 0):
        with rhs.hd.options(pair_persist=persist, pair_persist_s=S):
            p = p0.detach().clone().requires_grad_(True)
            x0 = u0.detach().clone().requires_grad_(True)
            sol = kanode.solve(rhs, x0, (0.0, 0.05), p, ts, opt, sensealg="interpolating_adjoint")
            g, gu = torch.autograd.grad((sol.u * w).sum(), [p, x0])
            out.append((g, gu, sol.stats))
            assert rhs.hd.get_option("last_adjoint") == (L.ADJ_PAIR_PERSIST if persist else L.ADJ_HOST_LOOP)
    (g1, gu1, s1), (g1b, gu1b, _), (g0, gu0, s0) = out
    assert torch.equal(g1, g1b) and torch.equal(gu1, gu1b)
    assert s1["adjoint"]["naccept"] == s0["adjoint"]["naccept"] and s1["adjoint"]["nreject"] == s0["adjoint"]["nreject"]
    bar = 1e-9 if adaptive else 1e-11
    assert (g1 - g0).abs().max().item() <= bar * g0.abs().max().item()
    assert (gu1 - gu0).abs().max().item() <= bar * gu0.abs().max().item()


@pytest.mark.parametrize("adaptive", [True, False])
def test_persistent_pair_adjoint_falls_back(adaptive):
    """VERDICT r4 #3 / ADVICE r4: the one-launch surrogate adjoint's workgroups spin on each other, so it runs
    only when all of them can be resident, and an exchange time-out re-runs the adjoint on the launch-per-stage
    path instead of failing the call.  Forced both ways on the Burgers [512, 10, 512] shape (64 workgroups):
    PAIR_PERSIST_MAX_WG = 8 (a device with room for 8 resident workgroups: the launch is refused up front) and
    PAIR_PERSIST_ABORT = 1 (the abort word raised at launch, as a time-out raises it: the kernel drains and
    the host re-runs).  Both give the launch path's gradient bitwise, and the handle then still takes the
    one-launch path when allowed.  KANODE_OPT_RECORD_ADJOINT_STEPS: every path records its accepted backward
    steps (the one-launch kernel from the device), which tile the span and agree between the paths."""
    N, G, B = 512, 5, 4
    chain = kanode.Chain(kanode.KDense(N, 10, G, normalizer="softsign"), kanode.KDense(10, N, G, normalizer="softsign"))
    rhs = kanode.ChainRHS(chain, device=device())
    x = np.linspace(-1.0, 1.0, N)
    a = np.random.default_rng(7).normal(0.0, 0.1, (B, 3))
    u0 = t(-np.sin(np.pi * x)[None, :] + sum(a[:, k:k + 1] * np.sin((k + 1) * np.pi * x)[None, :] for k in range(3)))
    p0 = t(chain.setup(np.random.default_rng(3))[0].astype(np.float64))
    ts = [0.0, 0.01, 0.02, 0.035, 0.05]
    w = torch.as_tensor(np.random.default_rng(4).normal(size=(len(ts),) + tuple(u0.shape)), device=device())
    opt = kanode.Tsit5Options() if adaptive else kanode.Tsit5Options(adaptive=False, dt=0.004)

    def grad(**o):
        with rhs.hd.options(**o):
            p = p0.detach().clone().requires_grad_(True)
            x0 = u0.detach().clone().requires_grad_(True)
            sol = kanode.solve(rhs, x0, (0.0, 0.05), p, ts, opt, sensealg="interpolating_adjoint")
            g, gu = torch.autograd.grad((sol.u * w).sum(), [p, x0])
            hs = np.asarray(sol.stats["adjoint"]["dts"])
            assert len(hs) == sol.stats["adjoint"]["naccept"] and abs(hs.sum() - 0.05) <= 1e-12
            return g, gu, rhs.hd.get_option("last_adjoint"), hs

    with rhs.hd.options(record_adjoint_steps=1):
        g0, gu0, path0, hs0 = grad(pair_persist=0)
        assert path0 == L.ADJ_HOST_LOOP
        gc, guc, pathc, hsc = grad(pair_persist_max_wg=8)
        assert pathc == L.ADJ_HOST_LOOP
        ga, gua, patha, hsa = grad(pair_persist_abort=1)
        assert patha == L.ADJ_PAIR_FALLBACK
        for g, gu, hs in ((gc, guc, hsc), (ga, gua, hsa)):
            assert torch.equal(g, g0) and torch.equal(gu, gu0) and np.array_equal(hs, hs0)
        g1, gu1, path1, hs1 = grad()
        assert path1 == L.ADJ_PAIR_PERSIST
    bar = 1e-9 if adaptive else 1e-11
    assert (g1 - g0).abs().max().item() <= bar * g0.abs().max().item()
    assert len(hs1) == len(hs0) and np.abs(hs1 / hs0 - 1).max() <= (1e-6 if adaptive else 1e-12)



@pytest.mark.parametrize("name", ["fk256", "lv64", "lv32"])
def test_dense_saveat_batches_per_step(name):
    """Many saveat stops per accepted step (round 4: a step's saveat values are one launch,
    kan::SaveatStep, at most 48 stops per launch): 4001 stops for LV (2000 per unit time, steps of
    ~0.05-0.2 hold 100+, so the batch flushes) and 601 over a short FK256 span, plus stops that land on step ends (copies of u_new).  Against
    the Python driver (one lincomb per stop): same steps, values to rounding.  lv64 / lv32 with the
    one-workgroup solve off (the host loop, K-form interpolation); fk256 on its fused step (Q form)."""
    rhs, u0, p, tspan, _ = _setup(name)
    tspan, n = ((0.0, 2.0), 4000) if name.startswith("lv") else ((0.0, 0.05), 600)
    ts = [tspan[0] + (tspan[1] - tspan[0]) * i / n for i in range(n + 1)]
    f64 = u0.dtype == torch.float64
    opt = kanode.Tsit5Options(abstol=1e-8 if f64 else 1e-6, reltol=1e-7 if f64 else 1e-4)
    with rhs.hd.options(fused_solve=0):
        nat = kanode.solve(rhs, u0, tspan, p, ts, opt)
        py = kanode.solve(rhs, u0, tspan, p, ts, dataclasses.replace(opt, native=False))
    assert nat.u.shape == py.u.shape == (n + 1,) + tuple(u0.shape)
    assert n > 4 * nat.stats["naccept"]                      # several stops per step
    scale = max(1.0, py.u.abs().max().item())
    if f64:
        assert nat.stats["naccept"] == py.stats["naccept"]
        assert (nat.u - py.u).abs().max().item() <= max(1e-11, 1e-3 * opt.reltol) * scale
    else:
        assert abs(nat.stats["naccept"] - py.stats["naccept"]) <= 2
        assert (nat.u - py.u).abs().max().item() <= 20 * opt.reltol * scale


@pytest.mark.parametrize("nx,B,G,norm", [(26, 1, 10, "softsign"), (64, 3, 10, "softsign"), (16, 16, 5, "tanh_fast"),
                                         (40, 5, 10, "tanh_fast")])
@pytest.mark.parametrize("adaptive", [True, False])
def test_fk_small_one_workgroup_matches_host_loop(nx, B, G, norm, adaptive):
    """the Fisher-KPP problem at the reference's own size (Fisher-KPP_Source.jl:34-49: 26 points,
    one IC) runs the whole forward solve and the whole InterpolatingAdjoint as one workgroup each
    (kan_small.hip: wave = trajectory, lane = grid point, KAN from the LDS tables) instead of the host loop's
    per-step launches.  Against the host loop (KANODE_OPT_FUSED_SOLVE = 0): the forward RHS is the same
    arithmetic per point (pp_pair_finish's order), so at fixed steps the saveat values are equal to the
    error-norm-free rounding (bitwise in practice); the adjoint's per-point pullback is the table one
    (pp_vjp_point) where the host loop at these Nx runs the recurrence kernel, both within 1e-14 of the
    derivative scale (test_gpu_pp.py), so the gradients agree to ~n_steps·1e-14.  Adaptive: the block-summed
    error norms round differently from the host loop's, so the step sizes differ at rounding level: the
    solutions agree to the tolerance, and where that leaves an accept/reject elsewhere (a stability-limited
    adjoint of a few hundred steps) the step counts to 1% and the gradients to 50·reltol (as
    test_native_adjoint_matches_python_adjoint)."""
    rhs = _fk_cfg(nx, G, norm)
    u0 = t(fk_u0(nx, B, 9))
    p0 = t(np.random.default_rng(nx + B).uniform(-1.0, 1.0, G + 1))
    ts = [0.0, 0.5, 1.0, 1.5, 2.0]
    opt = kanode.Tsit5Options(abstol=1e-9, reltol=1e-9) if adaptive else kanode.Tsit5Options(adaptive=False, dt=0.02)
    w = t(np.random.default_rng(5).normal(size=(len(ts),) + tuple(u0.shape)))
    out = []
    for fused in (1, 0):
        with rhs.hd.options(fused_solve=fused, record_adjoint_steps=1):
            p = p0.clone().requires_grad_(True)
            x0 = u0.clone().requires_grad_(True)
            sol = kanode.solve(rhs, x0, (0.0, 2.0), p, ts, opt, sensealg="interpolating_adjoint")
            g, gu = torch.autograd.grad((sol.u * w).sum(), [p, x0])
            out.append((sol.u.detach(), g, gu, sol.stats, rhs.hd.get_option("last_adjoint")))
    (u1, g1, gu1, s1, path1), (u0_, g0, gu0, s0, path0) = out
    assert path1 == L.ADJ_CHAIN_WG and path0 == L.ADJ_HOST_LOOP
    for st in (s1, s0):   # both record their backward steps (the one-workgroup kernel from the device)
        hs = np.asarray(st["adjoint"]["dts"])
        assert len(hs) == st["adjoint"]["naccept"] and abs(hs.sum() - 2.0) <= 1e-12
    scale = u0_.abs().max().item()
    if not adaptive:
        assert s1["naccept"] == s0["naccept"] and s1["adjoint"]["naccept"] == s0["adjoint"]["naccept"]
        assert (u1 - u0_).abs().max().item() <= 1e-13 * scale
        bar = 1e-11
    else:
        assert s1["naccept"] == s0["naccept"]
        assert (u1 - u0_).abs().max().item() <= 10 * opt.reltol * scale
        na, nb = s1["adjoint"]["naccept"], s0["adjoint"]["naccept"]
        assert abs(na - nb) <= 0.01 * nb
        bar = 1e-9 if na == nb else 50 * opt.reltol
    assert (g1 - g0).abs().max().item() <= bar * g0.abs().max().item()
    assert (gu1 - gu0).abs().max().item() <= bar * gu0.abs().max().item()


@pytest.mark.parametrize("adaptive", [True, False])
def test_two_layer_wide_adjoint_other_shapes(adaptive):
    """The whole-workgroup adjoint of one trajectory (kd_chain_adjoint_wide_kernel, WideModel) for two-layer
    chains other than the Lotka-Volterra shape (which runs on one wave, kd_chain_adjoint_lvwave_kernel):
    [3 -> 8 -> 3] G = 4 softsign, against the group kernel (KANODE_OPT_CHAIN_WIDE = 0) at 1e-10."""
    chain = kanode.Chain(kanode.KDense(3, 8, 4, normalizer="softsign"), kanode.KDense(8, 3, 4, normalizer="softsign"))
    rhs = kanode.ChainRHS(chain, device=device())
    p0 = chain.setup(np.random.default_rng(5))[0] / 10
    u0 = np.array([[0.5, -0.2, 0.8]])
    ts = [0.1 * i for i in range(11)]
    w = torch.as_tensor(np.random.default_rng(7).normal(size=(len(ts), 1, 3)), device=device())
    opt = kanode.Tsit5Options(abstol=1e-9, reltol=1e-9) if adaptive else kanode.Tsit5Options(adaptive=False, dt=0.02)
    out = []
    for wide in (1, 0):
        with rhs.hd.options(chain_wide=wide):
            p = torch.as_tensor(p0.astype(np.float64), device=device()).requires_grad_(True)
            x0 = torch.as_tensor(u0, device=device()).requires_grad_(True)
            sol = kanode.solve(rhs, x0, (0.0, 1.0), p, ts, opt, sensealg="interpolating_adjoint")
            out.append(torch.autograd.grad((sol.u * w).sum(), [p, x0]) + (sol.stats["adjoint"]["naccept"],))
            assert rhs.hd.get_option("last_adjoint") == L.ADJ_CHAIN_WG
    (gw, guw, nw), (gg, gug, ng) = out
    assert nw == ng
    for a_, b_ in ((gw, gg), (guw, gug)):
        assert (a_ - b_).abs().max().item() <= 1e-10 * b_.abs().max().item()


@pytest.mark.parametrize("adaptive", [True, False])
def test_lv1_wide_adjoint_matches_group_adjoint_and_oracle(adaptive):
    """one Lotka-Volterra trajectory (LV_driver_KANODE.jl:180-184,279-291, BASELINE configs[0])
    runs its adjoint on ONE wave (kd_chain_adjoint_lvwave_kernel: one basis function per lane, readlane /
    ds_bpermute for every cross-lane value, no barriers, every parameter cotangent one lane's product) instead
    of one 16-lane group.  Against the
    group kernel (KANODE_OPT_CHAIN_WIDE = 0) and against the Python driver over the CPU oracle chain: equal step
    counts, gradients to 1e-10 (the basis values come from the per-knot formula here and from the Gaussian
    recurrence in the group kernel, both within ~3e-15 of each other)."""
    from oracle_rhs import OracleChainRHS
    specs = [O.LayerSpec(2, 10, 5, "tanh_fast"), O.LayerSpec(10, 2, 5, "tanh_fast")]
    u0 = np.array([[1.0, 1.0]])
    p0 = kanode.Chain(kanode.KDense(2, 10, 5), kanode.KDense(10, 2, 5)).setup(np.random.default_rng(4))[0] / 10
    ts = [0.1 * i for i in range(35)]
    w = np.random.default_rng(6).normal(size=(len(ts), 1, 2))
    opt = kanode.Tsit5Options(abstol=1e-9, reltol=1e-9) if adaptive else kanode.Tsit5Options(adaptive=False, dt=0.01)

    def grad(f, dev):
        p = torch.as_tensor(p0.astype(np.float64), device=dev).requires_grad_(True)
        x0 = torch.as_tensor(u0, device=dev).requires_grad_(True)
        sol = kanode.solve(f, x0, (0.0, 3.5), p, ts, opt, sensealg="interpolating_adjoint")
        g, gu = torch.autograd.grad((sol.u * torch.as_tensor(w, device=dev)).sum(), [p, x0])
        return g.cpu(), gu.cpu(), sol.stats["adjoint"]["naccept"], np.asarray(sol.stats["adjoint"]["dts"])

    rhs = lv()
    rhs.hd.set_option("record_adjoint_steps", 1)
    gw, guw, nw, hw = grad(rhs, device())
    assert rhs.hd.get_option("last_adjoint") == L.ADJ_CHAIN_WG
    with rhs.hd.options(chain_wide=0):
        gg, gug, ng, hg = grad(rhs, device())
        assert rhs.hd.get_option("last_adjoint") == L.ADJ_CHAIN_WG
    gc, guc, nc, hc = grad(OracleChainRHS(specs), "cpu")
    assert nw == ng == nc == len(hw) == len(hg) == len(hc)
    for h_ in (hw, hg):   # the device-recorded backward steps against the driver's
        assert np.abs(h_ / hc - 1).max() <= (1e-6 if adaptive else 1e-12)
    for a_, b_ in ((gw, gg), (gw, gc), (guw, gug), (guw, guc)):
        assert (a_ - b_).abs().max().item() <= 1e-10 * b_.abs().max().item()


@pytest.mark.parametrize("dtype,B,shape", [(torch.float32, 4096, "lv"), (torch.float64, 300, "lv"),
                                            (torch.float64, 200, "chain3"), (torch.float64, 200, "chain3_mixed")])
@pytest.mark.parametrize("adaptive", [True, False])
def test_fused_chain_adjoint_step_matches_stage_launches(dtype, B, shape, adaptive):
    """VERDICT r5 #3 (BASELINE configs[1]: LV, 4,096 ICs, fp32): the host-loop InterpolatingAdjoint of a batched
    small chain takes each step as ONE kd_chain_vjp_step_kernel launch (the six stages per column in registers,
    each stage's kμ block sums into its own slab region) + one reduction launch, instead of six stage launches
    and six reductions.  Same per-column arithmetic, same blocks and reduction order: du0 and dp bitwise equal
    to the per-stage path (KANODE_OPT_FUSED_STEP = 0), with the same step sequence.  KANODE_OPT_LAST_EVAL says which
    launcher served the adjoint's last call: the step kernel under FUSED_STEP = 1 for LV and for chain3, a generic (not
    fixed-shape) chain of three layers under one normalizer.  chain3_mixed is the chain this test ran before, whose
    middle layer has another normalizer: chain_small_layers refuses it, so both settings run the per-layer kernels
    and the comparison holds trivially; it stays as the case whose expected path is per layer.  (With one normalizer
    its widths [3, 6, 5, 3] would still miss the step kernel in fp64: P = 315 needs 3·1248 + 315·8·29 = 76,824 B of
    the 65,536 B chain_vjp_step_supported allows.  chain3 is [3, 5, 4, 3], P = 235: 58,264 B.)"""
    if shape == "lv":
        rhs = lv(dtype)
    elif shape == "chain3_mixed":
        rhs = kanode.ChainRHS(kanode.Chain(kanode.KDense(3, 6, 4), kanode.KDense(6, 5, 4, normalizer="softsign"),
                                           kanode.KDense(5, 3, 4)), dtype=dtype, device=device())
    else:
        rhs = kanode.ChainRHS(kanode.Chain(kanode.KDense(3, 5, 4), kanode.KDense(5, 4, 4), kanode.KDense(4, 3, 4)),
                              dtype=dtype, device=device())
    want = {1: L.EVAL_PER_LAYER if shape == "chain3_mixed" else L.EVAL_CHAIN_ADJ_STEP,
            0: L.EVAL_PER_LAYER if shape == "chain3_mixed" else L.EVAL_CHAIN_KERNEL}
    N = rhs.N
    u0 = t(np.random.default_rng(5).uniform(0.5, 2.0, (B, N)), dtype)
    p0 = t(np.random.default_rng(7).uniform(-0.3, 0.3, rhs.P), dtype)
    ts = [0.1 * i for i in range(35)]
    w = t(np.random.default_rng(11).normal(size=(len(ts), B, N)), dtype)
    opt = kanode.Tsit5Options() if adaptive else kanode.Tsit5Options(adaptive=False, dt=0.05)
    res = {}
    for fused in (1, 0):
        with rhs.hd.options(fused_step=fused):
            p = p0.clone().requires_grad_(True)
            x0 = u0.clone().requires_grad_(True)
            sol = kanode.solve(rhs, x0, (0.0, 3.5), p, ts, opt, sensealg="interpolating_adjoint")
            gp, gu = torch.autograd.grad((sol.u * w).sum(), [p, x0])
            assert rhs.hd.get_option("last_eval") == want[fused]
            res[fused] = (gp, gu, sol.stats)
    (g1, u1, s1), (g0, u0_, s0) = res[1], res[0]
    assert s1["adjoint"]["naccept"] == s0["adjoint"]["naccept"] and s1["adjoint"]["nreject"] == s0["adjoint"]["nreject"]
    assert torch.equal(g1, g0)
    assert torch.equal(u1, u0_)


def test_lv4096_adjoint_matches_cpu_oracle():
    """The batched LV training gradient (configs[1]'s shape, fp64 here so the comparison is at the restatement's
    precision) against the C port of the same solve + InterpolatingAdjoint (oracle/cpu_epoch.c) on 512 of the ICs:
    equal step counts, gradient within 1e-9 of its scale."""
    B = 512
    rhs = lv(torch.float64)
    u0n = np.random.default_rng(1).uniform(0.5, 2.0, (B, 2))
    ts = [0.1 * i for i in range(35)]
    X = np.random.default_rng(2).uniform(0.5, 2.0, (35, B, 2))
    p0 = np.load(__import__("os").path.join(__import__("os").path.dirname(__import__("os").path.dirname(
        __import__("os").path.abspath(__file__))), "tests", "golden", "lv_trained_p_seed1.npy"))
    tr = kanode.Trainer(rhs, t(u0n), (0.0, 3.5), ts, t(X), t(p0), eta=5e-4)
    loss, g, sol = tr.loss_and_grad()
    specs = [O.LayerSpec(2, 10, 5, "tanh_fast"), O.LayerSpec(10, 2, 5, "tanh_fast")]
    lc, gc, _, st, _ = O.chain_epoch(specs, p0.copy(), u0n, 3.5, ts, X, eta=5e-4)
    assert sol.stats["naccept"] == st["naccept"] and sol.stats["adjoint"]["naccept"] == st["adjoint_naccept"]
    assert abs(float(loss) - lc) <= 1e-12 * lc
    assert np.abs(g.cpu().numpy() - gc).max() <= 1e-9 * np.abs(gc).max()
