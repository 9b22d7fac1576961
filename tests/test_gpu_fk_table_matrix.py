"""The Fisher-KPP table kernels of kan_pp.hip against the fp64 C oracle, over the case table of tests/fk_table_cases.py:
the pair kernels (short and long, with the batches that take their second and third trips), the wave RHS at NP = 1, 2,
4 with block tails of one row, a full block and a full block plus one, the persistent grid with several trips and a
ragged last one, the stage kernel with y_out and the error norm, the standalone VJP and the VJP stage on the four
table configurations (NI = 256 at compile time and the runtime-ni kernel), and the step, step-loop, adjoint-step
(rows and wave) and adjoint-loop kernels through the integrator in the form of test_gpu_fk_e2e.py.  Every record
asserts the launch kanode_last_fk_launch reports against the one stated for it, so a launcher that silently took
another kernel, grid, chunk, combine or finish fails here.

The pass criterion of a single-launch record is gpu_util.assert_close at RTOL[float64] under fk_table_cases.scales
(fk_cases.fk_error_scale plus the table's acceptance tolerance; test_fk_table_cases_cpu.py shows it sound and what it
discriminates).  Guards on every record: outputs live in buffers whose rows past B hold a NaN sentinel that must keep
its bits, inputs in buffers whose rows past B are NaN, results below B are finite, and the same call twice gives the
same bits.  The integrator records keep test_gpu_fk_e2e.py's bars: equal step counts, u to 1e-11, gradients to 1e-9
relative.

Every record prints its err/bound before it asserts.  The single-launch records run one test per group of
fk_table_cases.GROUPS (an operation at one nx), which reports every failing record by its id: 56 tests over the 905
records (24 groups and 32 integrator records), 14 s wall on an MI355X; none above 2.3 s.  Worst
err/bound measured there, per class: pair short du 0.0028, pair long 0.0060, wave RHS 0.0073; stage du 0.011 (y_out
0.37 and the error norm 0.0028 of their derived bounds); VJP λᵀJ 0.0080, dp 0.044; VJP stage λᵀJ 0.0086, dp 0.056
(lam_out 0.25, error norm 0.0070).  The integrator records, as fractions of their bars (u 1e-11, dp and du0 1e-9
relative): step + adjoint step rows 3.4e-4 / 7.4e-5 / 2.0e-5, the two device loops 3.3e-4 / 2.6e-6 / 1.2e-5, the
stage launches 1.4e-4 / 7.4e-5 / 1.6e-6, the wave adjoint step 0.027 / 7.4e-5 / 4.4e-6 (the 0.027 is the adaptive
span at nx = 512, where the oracle driver with one-ulp noise on its own du moves by 0.021 of the bar).  Every record
reported the launch stated for it."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import fk_table_cases as TC
from gpu_util import RTOL, assert_close, device, t
from oracle import oracle as O
from oracle.oracle_rhs import OracleFKRHS
from test_gpu_fk_e2e import D as E2E_D, _u0

import kanode
from kanode import _lib as L

pytestmark = pytest.mark.gpu

SOLVE_BY_ID = {c.id: c for c in TC.SOLVE_CASES}
F64 = torch.float64
EPS = float(np.finfo(np.float64).eps)


@functools.lru_cache(maxsize=None)
def _cus():
    return torch.cuda.get_device_properties(device()).multi_processor_count


@pytest.fixture(scope="module", autouse=True)
def _drop_handles():
    """The handles are shared by this module's records and destroyed when it ends."""
    yield
    _handle.cache_clear()


@functools.lru_cache(maxsize=None)
def _handle(variant, nx, diff):
    n, b, G = TC.VARIANTS[variant][:3]
    D, dx = TC.FC.DIFFUSION[diff](nx)
    rhs = kanode.FisherKPPRHS(kanode.LayerCfg(1, 1, G, n, b, True, (-1.0, 1.0), None, True), nx=nx, dx=dx, D=D,
                              dtype=F64, device=device())
    assert rhs.hd.pointwise_table
    return rhs.hd


def _in(a):
    """The array in a device buffer whose rows past its own are NaN; the view of its rows."""
    full = torch.full((a.shape[0] + TC.PAD, a.shape[1]), float("nan"), dtype=F64, device=device())
    full[:a.shape[0]] = t(a)
    return full[:a.shape[0]]


class _Out:
    """An output of B rows inside a buffer pre-filled with a NaN sentinel."""

    def __init__(self, B, nx):
        self.full = torch.full((B + TC.PAD, nx), float("nan"), dtype=F64, device=device())
        self.v = self.full[:B]
        self.B = B

    def check(self, what):
        tail = self.full[self.B:].view(torch.int64)
        sent = torch.full((1,), float("nan"), dtype=F64, device=device()).view(torch.int64)
        assert bool((tail == sent).all()), f"{what}: rows past B were written"
        assert bool(torch.isfinite(self.v).all()), f"{what}: a row below B is not finite"
        return self.v


def _ptr(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(device()).cuda_stream)


def _vjp(hd, p, u, lam, lamJ, dp):
    L.check(L.lib().kanode_vjp(hd._h, _ptr(p), _ptr(u), _ptr(lam), _ptr(lamJ), _ptr(dp), u.shape[0], _stream()),
            hd._h, "kanode_vjp")


def _vjp_stage(hd, p, u, ks, lam, lks, lam_out, sumsq, lamJ, dp):
    su = hd._stage_struct(ks, TC.STAGE_C)
    sl = hd._stage_struct(lks, TC.LSTAGE_C, lam_out, (TC.STAGE_EC, TC.ABSTOL, TC.RELTOL, sumsq))
    L.check(L.lib().kanode_vjp_stage(hd._h, _ptr(p), _ptr(u), C.byref(su), _ptr(lam), C.byref(sl), _ptr(lamJ),
                                     _ptr(dp), u.shape[0], _stream()), hd._h, "kanode_vjp_stage")


def _ratio(got, ref, scale):
    return float(np.max(np.abs(got.detach().cpu().numpy() - ref) / (RTOL[F64] * scale)))


def _said(hd, c):
    assert tuple(hd.last_fk_launch()) == c.launch.astuple(_cus()), (tuple(hd.last_fk_launch()), c.launch)


def _rhs_record(c, hd, d, r, B):
    p, u = t(d.p), _in(d.u)
    outs = []
    for _ in range(2):
        o = _Out(B, c.nx)
        hd.rhs(p, u, out=o.v)
        _said(hd, c)
        outs.append(o.check("du"))
    rows = TC.big_slice(c, _cus()) if c.B == "big" else np.arange(B)
    got = outs[0][torch.as_tensor(rows, device=device())]
    print(f"FKTABLE {c.id} {c.launch.family} du {_ratio(got, r.du, r.s_du):.3g}")
    assert_close(got, r.du, r.s_du, RTOL[F64], "du")
    assert torch.equal(outs[0], outs[1])
    if c.B == "big":        # trajectory independence across the trips: the batch equals its shards, bitwise
        k = B // 3 + 1
        parts = [hd.rhs(p, u[i:i + k]) for i in range(0, B, k)]
        assert torch.equal(outs[0], torch.cat(parts))


def _stage_record(c, hd, d, r, B):
    p, u, ks = t(d.p), _in(d.u), [_in(k) for k in d.ks]
    res = []
    for _ in range(2):
        du, y = _Out(B, c.nx), _Out(B, c.nx)
        sumsq = torch.full((1,), float("nan"), dtype=F64, device=device())
        hd.rhs_stage(p, u, ks, TC.STAGE_C, y_out=y.v, error=(TC.STAGE_EC, TC.ABSTOL, TC.RELTOL, sumsq), out=du.v)
        _said(hd, c)
        res.append((du.check("du"), y.check("y_out"), sumsq))
    du, y, sumsq = res[0]
    # y_out: the kernel's fma chain against the sum rounded once: one rounding per term of Σ|terms|
    ys = (len(d.ks) + 1) * EPS * (np.abs(d.u) + sum(abs(cj) * np.abs(k) for cj, k in zip(TC.STAGE_C, d.ks)))
    eq = abs(sumsq.item() - r.err) / r.err_bound
    print(f"FKTABLE {c.id} stage du {_ratio(du, r.du, r.s_du):.3g} y {_ratio(y, r.y, ys / RTOL[F64]):.3g} err {eq:.3g}")
    assert_close(du, r.du, r.s_du, RTOL[F64], "du")
    assert_close(y, r.y, ys, 1.0, "y_out")
    assert eq <= 1.0, f"error norm: err/bound {eq:.3g}"
    assert all(torch.equal(a, b) for a, b in zip(res[0], res[1]))


def _vjp_record(c, hd, d, r, B):
    stage = c.op == "vjp_stage"
    p, u, lam = t(d.p), _in(d.u), _in(d.lam)
    ks = [_in(k) for k in d.ks] if stage else None
    lks = [_in(k) for k in d.lks] if stage else None

    def call(dp, want_lamJ=True):
        lamJ, ls = _Out(B, c.nx), _Out(B, c.nx)
        sumsq = torch.full((1,), float("nan"), dtype=F64, device=device())
        if stage:
            _vjp_stage(hd, p, u, ks, lam, lks, ls.v, sumsq, lamJ.v, dp)
        else:
            _vjp(hd, p, u, lam, lamJ.v if want_lamJ else None, dp)
        _said(hd, c)
        if not want_lamJ:
            assert bool((lamJ.full.view(torch.int64) == lamJ.full.view(torch.int64)[0, 0]).all())
            return None
        return lamJ.check("lamJ"), (ls.check("lam_out") if stage else None), sumsq

    dp = torch.zeros_like(p)
    lamJ, ls, sumsq = call(dp)
    msg = (f"FKTABLE {c.id} {c.launch.family} lamJ {_ratio(lamJ, r.lamJ, r.s_lamJ):.3g} "
           f"dp {_ratio(dp, r.dp, r.s_dp):.3g}")
    if stage:
        lss = (len(d.lks) + 1) * EPS * (np.abs(d.lam) + sum(abs(cj) * np.abs(k) for cj, k in zip(TC.LSTAGE_C, d.lks)))
        eq = abs(sumsq.item() - r.err) / r.err_bound
        msg += f" ls {_ratio(ls, r.ls, lss / RTOL[F64]):.3g} err {eq:.3g}"
    print(msg)
    assert_close(lamJ, r.lamJ, r.s_lamJ, RTOL[F64], "lamJ")
    assert_close(dp, r.dp, r.s_dp, RTOL[F64], "dp")
    assert bool(torch.isfinite(dp).all())
    if stage:
        assert_close(ls, r.ls, lss, 1.0, "lam_out")
        assert eq <= 1.0, f"λ error norm: err/bound {eq:.3g}"
    dp2 = torch.zeros_like(p)
    lamJ2, ls2, sumsq2 = call(dp2)
    assert torch.equal(lamJ2, lamJ) and torch.equal(dp2, dp) and (not stage or torch.equal(sumsq2, sumsq))
    if not stage:       # a dp-only call (lam_J = NULL) gives the full call's dp
        dp3 = torch.zeros_like(p)
        call(dp3, want_lamJ=False)
        assert torch.equal(dp3, dp)
    dp0 = np.random.default_rng(c.seed + 1).normal(size=d.p.shape)      # dp accumulates into a non-zero buffer
    dp4 = t(dp0)
    call(dp4)
    g = dp.cpu().numpy()
    assert_close(dp4, dp0 + g, RTOL[F64] * r.s_dp + 2 * EPS * (np.abs(dp0) + np.abs(g)), 1.0, "dp0 + dp")


@pytest.mark.parametrize("gid", list(TC.GROUPS))
def test_records(gid):
    """Every record of the group (fk_table_cases.GROUPS: one operation at one nx); each failing record is reported by
    its id.  Only a failed assertion is collected: a HIP error ends the test at once."""
    failed = []
    for c in TC.GROUPS[gid]:
        try:
            _record(c)
        except AssertionError as e:
            failed.append(f"{c.id}: {str(e).splitlines()[0] if str(e) else 'assert'}")
    assert not failed, f"{len(failed)} of {len(TC.GROUPS[gid])} records: " + "; ".join(failed[:8])


def _record(c):
    B = c.rows(_cus())
    d = c.data(_cus())
    r = TC.reference(c, d, TC.big_slice(c, _cus()) if c.B == "big" else None)
    hd = _handle(c.variant, c.nx, c.diff)
    with hd.options(**c.opt):
        {"rhs": _rhs_record, "stage": _stage_record, "vjp": _vjp_record, "vjp_stage": _vjp_record}[c.op](c, hd, d, r, B)


def _run(f, dev, u0, p0, tspan, ts, w, opt, between=None):
    p = torch.as_tensor(p0, device=dev).clone().requires_grad_(True)
    x0 = torch.as_tensor(u0, device=dev).clone().requires_grad_(True)
    sol = kanode.solve(f, x0, tspan, p, ts, opt, sensealg="interpolating_adjoint")
    if between:
        between()
    gp, gu = torch.autograd.grad((sol.u * torch.as_tensor(w, device=dev)).sum(), [p, x0])
    return sol.u.detach().cpu(), gp.cpu(), gu.cpu(), sol.stats


@pytest.mark.parametrize("cid", list(SOLVE_BY_ID))
def test_solve_record(cid):
    """test_gpu_fk_e2e._e2e shortened to 4 fixed steps (or its short adaptive span), with its bars, and the launch
    record read after the forward solve and after the adjoint."""
    c = SOLVE_BY_ID[cid]
    nx, B, G = c.nx, c.B, c.G
    norm, basis = TC.VARIANTS[c.variant][:2]
    dx = 1.0 / (nx - 1)
    # (a LayerCfg, not KDense: KDense turns tanh into tanh_fast, and the runtime class needs the exact tanh)
    gpu = kanode.FisherKPPRHS(kanode.LayerCfg(1, 1, G, norm, basis, True, (-1.0, 1.0), None, True), nx=nx, dx=dx,
                              D=E2E_D, device=device())
    assert gpu.hd.pointwise_table
    cpu = OracleFKRHS(O.LayerSpec(1, 1, G, norm), E2E_D, dx, dense=True)
    seed = nx + B + G
    u0 = _u0(nx, B, seed)
    p0 = np.random.default_rng(seed + 100).uniform(-1.0, 1.0, G + 1)
    if c.mode == "fixed":
        dt = 5e-4 * (256 / nx) ** 2
        tspan, ts = (0.0, 4 * dt), [0.0, dt, 3 * dt, 4 * dt]
        opt = kanode.Tsit5Options(adaptive=False, dt=dt)
    else:
        T = 0.02 * (256 / nx) ** 2
        tspan, ts = (0.0, T), [0.0, 0.3 * T, 0.5 * T, T]
        opt = kanode.Tsit5Options(abstol=1e-9, reltol=1e-9)
    w = np.random.default_rng(seed + 200).normal(size=(len(ts), B, nx))
    seen = []
    with gpu.hd.options(**c.opt):
        ug, gg, gug, sg = _run(gpu, device(), t(u0), p0, tspan, ts, w, opt,
                               lambda: seen.append(tuple(gpu.hd.last_fk_launch())))
        seen.append(tuple(gpu.hd.last_fk_launch()))
    uc, gc, guc, sc = _run(cpu, "cpu", torch.as_tensor(u0), p0, tspan, ts, w, opt)
    eu = (ug - uc).abs().max().item()
    eg = (gg - gc).abs().max().item() / gc.abs().max().item()
    egu = (gug - guc).abs().max().item() / guc.abs().max().item()
    print(f"FKTABLE {cid} steps {sg['naccept']}+{sg['nreject']} / {sg['adjoint']['naccept']}+{sg['adjoint']['nreject']}"
          f" u {eu / 1e-11:.3g} dp {eg / 1e-9:.3g} du0 {egu / 1e-9:.3g} launches {seen}")
    assert seen[0] == c.fwd.astuple(_cus()), (seen[0], c.fwd)
    assert seen[1] == (c.adj or c.fwd).astuple(_cus()), (seen[1], c.adj)
    assert (sg["naccept"], sg["nreject"]) == (sc["naccept"], sc["nreject"])
    assert (sg["adjoint"]["naccept"], sg["adjoint"]["nreject"]) == (sc["adjoint"]["naccept"], sc["adjoint"]["nreject"])
    assert sg["naccept"] == 4 if c.mode == "fixed" else sg["naccept"] >= 5
    assert eu <= 1e-11
    assert eg <= 1e-9 and egu <= 1e-9
