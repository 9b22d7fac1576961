"""The per-point Fisher-KPP kernels of kan_fk.hip (fk_rhs_kernel, fk_vjp_kernel) against the fp64 C oracle, over the
case table of tests/fk_cases.py: the six instantiations launch_fk_rhs / launch_fk_vjp can pick (five in fp32), each
basis path with and without the base term, the pair / odd and short / long launches, a grid-stride launch of both
kernels, both dtypes, and the normalizer / basis / grid / denominator variants the ABI accepts, each at D = 0 (the KAN
part alone) and at D = dx² (Laplacian coefficient 1).  The pass criterion is gpu_util.assert_close at the project's
two RTOL values under fk_cases.fk_error_scale (test_fk_cases_cpu.py shows that scale sound and what it discriminates);
the reference of an fp32 record is the fp64 oracle at the fp32-rounded inputs.  An fp64 handle has the pointwise table
off, so that an even nx reaches these kernels too.

Every record prints its err/bound (du / λᵀJ / dp) before it asserts.  Measured on an MI355X, worst per path: fp64 direct
0.0022 / 0.0018 / 0.013, rec 0.0027 / 0.0029 / 0.044, rec_corr 0.0051 / 0.0043 / 0.031; fp32 direct 0.037 / 0.032 /
0.035, rec 0.032 / 0.029 / 0.037, rec_corr 0.021 / 0.059 / 0.040."""
import ctypes as C

import numpy as np
import pytest
import torch

import fk_cases as FC
from gpu_util import RTOL, assert_close, device, t
from oracle import oracle as O
from oracle_rhs import OracleFKRHS

import kanode

pytestmark = pytest.mark.gpu

BY_ID = {c.id: c for c in FC.CASES}
TDT = {"f64": torch.float64, "f32": torch.float32}
ALL = list(BY_ID)


def _make(c):
    n, b, G, lims, den, quirk, base, _, _ = FC.VARIANTS[c.variant]
    D, dx = c.D_dx
    rhs = kanode.FisherKPPRHS(kanode.LayerCfg(1, 1, G, n, b, base, lims, den, quirk), nx=c.nx, dx=dx,
                              D=D, dtype=TDT[c.dtype], device=device(), table=False if c.table_off else None)
    assert not rhs.hd.pointwise_table
    return rhs.hd


def _f64(x):
    return x.detach().double().cpu().numpy()


def _ratio(got, ref, scale, rtol):
    return float(np.max(np.abs(_f64(got) - ref) / (rtol * scale)))


@pytest.mark.parametrize("cid", ALL)
def test_record(cid):
    """du, λᵀJ and dp against the oracle; the same inputs twice give the same bits; a dp-only call (lam_J = NULL: λᵀJ
    goes to the handle workspace) equals the full call's dp bitwise; dp accumulates into a non-zero buffer (dp0 + dp
    to the bound of dp and the addition's rounding)."""
    c = BY_ID[cid]
    dt, rtol = TDT[c.dtype], RTOL[TDT[c.dtype]]
    p, u, lam = c.data()
    rdu, rlj, rdp = FC.oracle(c, p, u, lam)
    sdu, slj, sdp = FC.fk_error_scale(c, p, u, lam)
    hd = _make(c)
    pt, ut, lt = t(p, dt), t(u, dt), t(lam, dt)
    du = hd.rhs(pt, ut)
    lamJ, dp = hd.vjp(pt, ut, lt)
    print(f"FKMATRIX {cid} {c.dtype} {c.path} {_ratio(du, rdu, sdu, rtol):.3g} {_ratio(lamJ, rlj, slj, rtol):.3g} "
          f"{_ratio(dp, rdp, sdp, rtol):.3g}")
    assert_close(du, rdu, sdu, rtol, "du")
    assert_close(lamJ, rlj, slj, rtol, "lamJ")
    assert_close(dp, rdp, sdp, rtol, "dp")
    lamJ2, dp2 = hd.vjp(pt, ut, lt)
    assert torch.equal(hd.rhs(pt, ut), du) and torch.equal(lamJ2, lamJ) and torch.equal(dp2, dp)
    none, dp3 = hd.vjp(pt, ut, lt, want_lamJ=False)
    assert none is None and torch.equal(dp3, dp)
    dp0 = np.random.default_rng(c.seed + 1).normal(size=p.shape).astype(c.np_dtype()).astype(np.float64)
    _, dp4 = hd.vjp(pt, ut, lt, dp=t(dp0, dt))
    eps = float(torch.finfo(dt).eps)
    assert_close(dp4, dp0 + _f64(dp), rtol * sdp + 2 * eps * (np.abs(dp0) + np.abs(_f64(dp))), 1.0, "dp0 + dp")


# a handful of records for the properties below: each path in both dtypes, pair / odd, short / long
REPS = [f"{v}-{dt}-nx{nx}-B5-Ddx2" for dt in ("f64", "f32")
        for v, nx in (("softsign_rbf_G10", 26), ("softsign_rbf_G5", 5), ("softsign_rbf_G7", 257), ("tanh_rswaf_G5", 514),
                      ("tanhfast_rbf_G5", 255))]


@pytest.mark.parametrize("cid", REPS)
def test_batch_equals_its_shards(cid):
    """Trajectory independence: du and λᵀJ of a batch equal the concatenation of its shards', bitwise."""
    c = BY_ID[cid]
    dt = TDT[c.dtype]
    p, u, lam = c.data()
    hd = _make(c)
    pt, ut, lt = t(p, dt), t(u, dt), t(lam, dt)
    du = hd.rhs(pt, ut)
    lamJ, _ = hd.vjp(pt, ut, lt)
    parts = [(ut[:2].contiguous(), lt[:2].contiguous()), (ut[2:].contiguous(), lt[2:].contiguous())]
    assert torch.equal(du, torch.cat([hd.rhs(pt, a) for a, _ in parts]))
    assert torch.equal(lamJ, torch.cat([hd.vjp(pt, a, b)[0] for a, b in parts]))


@pytest.mark.parametrize("cid", [r for r in REPS if "-f32-" in r])
def test_host_variants_fp32(cid):
    """kanode_rhs_host / kanode_vjp_host on an fp32 handle equal the device calls bitwise."""
    c = BY_ID[cid]
    p, u, lam = (a.astype(np.float32) for a in c.data())
    hd = _make(c)
    lib = kanode.lib()
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    du = np.zeros_like(u)
    assert lib.kanode_rhs_host(hd._h, ptr(p), ptr(u), ptr(du), c.B) == 0
    pt, ut, lt = (t(a, torch.float32) for a in (p, u, lam))
    assert np.array_equal(du, hd.rhs(pt, ut).cpu().numpy())
    lamJ, dp = np.zeros_like(u), np.zeros_like(p)
    assert lib.kanode_vjp_host(hd._h, ptr(p), ptr(u), ptr(lam), ptr(lamJ), ptr(dp), c.B) == 0
    rJ, rdp = hd.vjp(pt, ut, lt)
    assert np.array_equal(lamJ, rJ.cpu().numpy()) and np.array_equal(dp, rdp.cpu().numpy())


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("cid", REPS)
def test_nonfinite_entry_stays_local(cid, bad):
    """One non-finite u entry reaches du only at its own point and its two periodic neighbours, λᵀJ only at its own
    point (the Laplacian there acts on λ); every other entry keeps its bits.  Asked at the first, the last and a
    middle point of the second trajectory."""
    c = BY_ID[cid]
    dt = TDT[c.dtype]
    p, u, lam = c.data()
    hd = _make(c)
    pt, ut, lt = t(p, dt), t(u, dt), t(lam, dt)
    du = hd.rhs(pt, ut)
    lamJ, _ = hd.vjp(pt, ut, lt)
    assert torch.isfinite(du).all() and torch.isfinite(lamJ).all()
    for i in (0, c.nx // 2, c.nx - 1):
        u2 = ut.clone()
        u2[1, i] = bad
        du2 = hd.rhs(pt, u2)
        lamJ2, _ = hd.vjp(pt, u2, lt)
        near = torch.zeros_like(ut, dtype=torch.bool)
        near[1, [(i - 1) % c.nx, i, (i + 1) % c.nx]] = True
        own = torch.zeros_like(near)
        own[1, i] = True
        assert not torch.isfinite(du2[1, i])
        assert torch.equal(du2[~near], du[~near]) and torch.equal(lamJ2[~own], lamJ[~own])


@pytest.mark.parametrize("variant", ["softsign_rbf_G5", "softsign_rbf_G10"])
def test_fp32_solve_and_adjoint_match_the_oracle_driver(variant):
    """kanode_solve_tsit5 + kanode_adjoint_tsit5 on an fp32 pointwise handle (solve_t<float> over these kernels: the
    recurrence at G = 5, the runtime-G direct kernel at G = 10) against the Python driver on the fp64 oracle with the
    dense Laplacian: nx = 26, B = 2, 20 fixed steps, four saveat stops.  The bar is derived as for the full-size
    surrogate adjoints: every RHS / VJP the GPU evaluates is within RTOL[fp32] of its scale of the
    oracle's (test_record), the solution is a sum of nf such evaluations times h and the gradients a sum of the
    adjoint's nf stage VJPs times h, and T·Lipschitz < 1 over this span (4·D/dx² = 25, |KAN'| about 3, T = 0.03), so
    both stay within nf·RTOL[fp32] of their size; the fp32 state updates add 20 roundings of 6e-8, far inside it.
    Measured on an MI355X: relative errors 3.8e-7 (u), 3.1e-7 (dp), 2.9e-7 (du0) at most against bars of 6.1e-4 and
    6.2e-4 (nf = 121 / 123), a ratio of 6e-4."""
    nx, B, D, dx, T, dt_step = 26, 2, 0.01, 1.0 / 25, 0.03, 0.0015
    n, b, G, lims, den, quirk, base, _, _ = FC.VARIANTS[variant]
    gpu = kanode.FisherKPPRHS(kanode.LayerCfg(1, 1, G, n, b, base, lims, den, quirk), nx=nx, dx=dx, D=D,
                              dtype=torch.float32, device=device())
    cpu = OracleFKRHS(O.LayerSpec(1, 1, G, n, b, base, lims, den, quirk), D, dx, dense=True)
    rng = np.random.default_rng(G)
    x = np.arange(nx) * dx
    ctr, wid, amp = rng.uniform(0.3, 0.7, (B, 1)), rng.uniform(0.1, 0.3, (B, 1)), rng.uniform(0.5, 1.0, (B, 1))
    f32 = lambda a: a.astype(np.float32).astype(np.float64)   # noqa: E731
    u0 = f32(amp * (np.tanh((x - (ctr - wid / 2)) / (wid / 10)) - np.tanh((x - (ctr + wid / 2)) / (wid / 10))) / 2)
    p0 = f32(rng.uniform(-1.0, 1.0, G + 1))
    ts = [0.0, 5 * dt_step, 12 * dt_step, T]
    w = f32(rng.normal(size=(len(ts), B, nx)))
    opt = kanode.Tsit5Options(adaptive=False, dt=dt_step)
    res = []
    for f, dev, tdt in ((gpu, device(), torch.float32), (cpu, "cpu", torch.float64)):
        p = torch.as_tensor(p0, dtype=tdt, device=dev).requires_grad_(True)
        x0 = torch.as_tensor(u0, dtype=tdt, device=dev).requires_grad_(True)
        sol = kanode.solve(f, x0, (0.0, T), p, ts, opt, sensealg="interpolating_adjoint")
        gp, gu = torch.autograd.grad((sol.u * torch.as_tensor(w, dtype=tdt, device=dev)).sum(), [p, x0])
        res.append((sol.u.detach().double().cpu(), gp.double().cpu(), gu.double().cpu(), sol.stats))
    (ug, gg, gug, sg), (uc, gc, guc, sc) = res
    assert sg["naccept"] == sc["naccept"] == 20 and sg["adjoint"]["naccept"] == sc["adjoint"]["naccept"]
    rel = lambda a_, b_: (a_ - b_).abs().max().item() / b_.abs().max().item()   # noqa: E731
    bar_u = RTOL[torch.float32] * sc["nf"]
    bar_g = RTOL[torch.float32] * sc["adjoint"]["nf"]
    eu, eg, egu = rel(ug, uc), rel(gg, gc), rel(gug, guc)
    print(f"FKSOLVE {variant}: nf {sc['nf']} / {sc['adjoint']['nf']}, rel err u {eu:.2e} (bar {bar_u:.1e}), "
          f"dp {eg:.2e}, du0 {egu:.2e} (bar {bar_g:.1e})")
    assert eu <= bar_u
    assert eg <= bar_g and egu <= bar_g
