"""The small-chain kernels of kan_col.hip (kd_chain_col_kernel, kd_chain_vjp_stage_kernel + chain_vjp_finish_kernel,
kd_chain_step_kernel, kd_chain_vjp_step_kernel) against the fp64 C oracle, over the case table of tests/chain_cases.py:
every rung of chain_ladder in both dtypes, the widths up to kChainDim, one to eight layers, N_in != N_out, both sides
of the two LDS budgets and of the forward kernel's batch cap, the pullback's single block, finish launch and second
loop trip, and the chains the launchers refuse on purpose.  After every call KANODE_OPT_LAST_EVAL has to name the
launcher the record states: a launcher that declines hands the call on without an error, so a comparison alone cannot
tell which path it checked.

The pass criterion is gpu_util.assert_close at the project's two RTOL values under the scales of layer_cases.py as they
stand: the chain scale against the oracle and between the chain kernels and the layer calls (other hidden bits), the
single-layer scale for every layer call at exact inputs; bitwise where two calls run the same launches.
test_chain_cases_cpu.py shows the table reaches what it claims, the scales sound and what they discriminate.  One
handle per row and dtype and one oracle evaluation per record, shared by the tests."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import chain_cases as CC
import layer_cases as LC
from gpu_util import RTOL, assert_close, cfgs_from_specs, device, t
from oracle import oracle as O

import kanode

pytestmark = pytest.mark.gpu

BY_ID = {c.id: c for c in CC.CASES}
TDT = {"f64": torch.float64, "f32": torch.float32}
ALL = [c.id for c in CC.CASES if not c.row.fwd_only]
FWD_ONLY = [c.id for c in CC.CASES if c.row.fwd_only]
# the pullback's single block (B = 4, or 1 where the row has no 4), its finish launch (5) and its second trip (4099)
ACCUMULATE = [c.id for c in CC.CASES if not c.row.fwd_only and c.B in ((4, 5, 4099) if 4 in c.row.batches else (1, 5))]
# square records on either side of the two kernels' one-block launches: 4 / 5 (pullback), 16 / 17 (forward)
STAGES = [c.id for c in CC.CASES if c.square and not c.row.fwd_only
          and c.B in ((4, 5, 16, 17) if 4 in c.row.batches else (5, 17))]
# the fused steps: chain_cases.ADJ_STEP's rows (one generic two-layer record per rung plus LV, and two past the fused
# adjoint step's LDS in fp64), at B = 17
STEPS = [f"{n}-{dt}-B{CC.STEP_B}" for n in CC.ADJ_STEP for dt in ("f64", "f32")]


@functools.lru_cache(maxsize=None)
def _handle(row_name, dtype):
    specs = BY_ID[f"{row_name}-{dtype}-B{CC.BY_NAME[row_name].batches[0]}"].specs()
    return kanode.KanodeHandle(cfgs_from_specs(specs), dtype=TDT[dtype], rhs_kind="chain", device=device())


@functools.lru_cache(maxsize=None)
def _ctx(cid):
    c = BY_ID[cid]
    dt = TDT[c.dtype]
    p, u, yb = c.data()
    specs = c.specs()
    for a in (p, u, yb):
        a.setflags(write=False)
    offs = np.cumsum([0] + [s.param_length() for s in specs])
    return SimpleNamespace(c=c, dt=dt, rtol=RTOL[dt], specs=specs, hd=_handle(c.row.name, c.dtype), p=p, u=u, yb=yb,
                           offs=offs, pt=t(p.copy(), dt), ut=t(u.copy(), dt), lt=t(yb.copy(), dt))


@functools.lru_cache(maxsize=None)
def _oracle(cid):
    """(y, x̄, p̄) of the oracle and the three chain scales."""
    x = _ctx(cid)
    y = O.chain_fwd(x.specs, x.p, x.u)
    xb, pb = O.chain_vjp(x.specs, x.p, x.u, x.yb)
    out = (y, xb, pb) + LC.chain_error_scale(x.specs, x.p, x.u, x.yb)
    for a in out:
        a.setflags(write=False)
    return out


def _f64(x):
    return x.detach().double().cpu().numpy()


def _last(hd):
    return hd.get_option("last_eval")


def _worst(got, ref, scale, rtol):
    return float(np.max(np.abs(_f64(got) - ref) / (rtol * scale)))


@pytest.mark.parametrize("cid", ALL)
def test_rhs_vjp_and_the_path_taken(cid):
    """rhs, λᵀJ and dp against the oracle under the chain scale; after each call last_eval names the launcher the
    record states; a repeated call is bitwise equal; the dp-only call (no λᵀJ) runs layer by layer whatever the shape
    (vjp_t) and is held to the same bound."""
    x = _ctx(cid)
    hd, c = x.hd, x.c
    y, xb, pb, ys, xs, ps = _oracle(cid)
    got = hd.rhs(x.pt, x.ut)
    assert _last(hd) == c.rhs_path
    lamJ, dp = hd.vjp(x.pt, x.ut, x.lt)
    assert _last(hd) == c.vjp_path
    print(f"{cid}: err/bound y {_worst(got, y, ys, x.rtol):.3g} xbar {_worst(lamJ, xb, xs, x.rtol):.3g} "
          f"pbar {_worst(dp, pb, ps, x.rtol):.3g}")
    assert_close(got, y, ys, x.rtol, "y")
    assert_close(lamJ, xb, xs, x.rtol, "xbar")
    assert_close(dp, pb, ps, x.rtol, "pbar")
    assert torch.equal(hd.rhs(x.pt, x.ut), got)
    lamJ2, dp2 = hd.vjp(x.pt, x.ut, x.lt)
    assert torch.equal(lamJ2, lamJ) and torch.equal(dp2, dp)
    none, dp3 = hd.vjp(x.pt, x.ut, x.lt, want_lamJ=False)
    assert none is None and _last(hd) == CC.EVAL_PER_LAYER
    assert_close(dp3, pb, ps, x.rtol, "pbar (dp only)")
    if not c.cls.vjp:
        assert torch.equal(dp3, dp)      # the same launches


@pytest.mark.parametrize("cid", FWD_ONLY)
def test_forward_batch_edge(cid):
    """K = 32,768 is the forward kernel's last batch, 32,769 runs layer by layer: the result against the oracle on
    either side, and the path."""
    x = _ctx(cid)
    y = O.chain_fwd(x.specs, x.p, x.u)
    # the chain scale's forward part (no pullback at this batch)
    Ls = LC.np_layers(x.specs)
    xs_, dxs = x.u, np.zeros_like(x.u)
    for l, lay in enumerate(Ls):
        pl = x.p[x.offs[l]:x.offs[l + 1]]
        dxs = LC._fwd_scale(lay, pl, xs_, dxs)
        xs_ = lay.fwd(pl, xs_)
    got = x.hd.rhs(x.pt, x.ut)
    assert _last(x.hd) == x.c.rhs_path
    assert_close(got, y, LC._floor(dxs), x.rtol, "y")
    assert torch.equal(x.hd.rhs(x.pt, x.ut), got)


@pytest.mark.parametrize("cid", ACCUMULATE)
def test_dp_accumulates(cid):
    """A second VJP onto a given dp0 gives dp0 + dp to rounding (the bound of dp, and the addition's rounding): the
    single block adds into dp itself, the finish launch adds the slab's sum."""
    x = _ctx(cid)
    ps = _oracle(cid)[5]
    rng = np.random.default_rng(x.c.seed + 1)
    dp0 = rng.normal(size=x.p.shape).astype(x.c.np_dtype()).astype(np.float64)
    _, dp = x.hd.vjp(x.pt, x.ut, x.lt)
    _, dp2 = x.hd.vjp(x.pt, x.ut, x.lt, dp=t(dp0, x.dt))
    assert _last(x.hd) == x.c.vjp_path
    eps = float(torch.finfo(x.dt).eps)
    assert_close(dp2, dp0 + _f64(dp), x.rtol * ps + 2 * eps * (np.abs(dp0) + np.abs(_f64(dp))), 1.0, "dp0 + dp")


@pytest.mark.parametrize("cid", [i for i in ALL if BY_ID[i].B <= 17])
def test_layer_by_layer(cid):
    """kanode_layer_forward / kanode_layer_vjp of every layer against O.layer_fwd / O.layer_vjp at the layer inputs
    and cotangents the GPU itself produced (exact inputs: the single-layer scale), and the chain's rhs / vjp against
    the composition of the layer calls: bitwise where the chain call runs layer by layer, under the chain scale where
    a one-launch kernel serves it (other summation order, other hidden bits)."""
    x = _ctx(cid)
    hd, specs, c = x.hd, x.specs, x.c
    _, _, _, ys, xs, ps = _oracle(cid)
    pl = [x.pt[x.offs[l]:x.offs[l + 1]].contiguous() for l in range(len(specs))]
    pl64 = [x.p[x.offs[l]:x.offs[l + 1]] for l in range(len(specs))]
    hs = [x.ut]
    for l in range(len(specs)):
        hs.append(hd.layer_forward(l, pl[l], hs[l]))
        assert _last(hd) == CC.EVAL_PER_LAYER
    g = x.lt
    pbs = [None] * len(specs)
    for l in range(len(specs) - 1, -1, -1):
        h64, g64 = _f64(hs[l]), _f64(g)
        xb, pb = hd.layer_vjp(l, pl[l], hs[l], g)
        sy, sx, sp = LC.layer_error_scale(specs[l], pl64[l], h64, g64)
        rxb, rpb = O.layer_vjp(specs[l], pl64[l], h64, g64)
        assert_close(hs[l + 1], O.layer_fwd(specs[l], pl64[l], h64), sy, x.rtol, f"layer {l} y")
        assert_close(xb, rxb, sx, x.rtol, f"layer {l} xbar")
        assert_close(pb, rpb, sp, x.rtol, f"layer {l} pbar")
        pbs[l] = pb
        g = xb
    y = hd.rhs(x.pt, x.ut)
    if c.cls.fwd:
        assert_close(y, _f64(hs[-1]), ys, x.rtol, "rhs against the layer calls")
    else:
        assert torch.equal(y, hs[-1])
    lamJ, dp = hd.vjp(x.pt, x.ut, x.lt)
    if c.cls.vjp:
        assert_close(lamJ, _f64(g), xs, x.rtol, "xbar against the layer calls")
        assert_close(dp, _f64(torch.cat(pbs)), ps, x.rtol, "pbar against the layer calls")
    else:
        assert torch.equal(lamJ, g) and torch.equal(dp, torch.cat(pbs))


@pytest.mark.parametrize("n_prev,n_adj", [(0, 0), (6, 5)])
@pytest.mark.parametrize("cid", STAGES)
def test_stages(cid, n_prev, n_adj):
    """kanode_rhs_stage (0 and 6 previous stages, y_out, error sum: the single block's own total at B <= 16, the slab
    and the final launch above) and kanode_vjp_stage (0 and 5 adjoint stages, lam_out) against rhs / vjp at the stage
    inputs they wrote out, and against the oracle there: bitwise where both run layer by layer, within the chain
    scale where a one-launch kernel serves either; the error sum against torch's to 1e-12 relative."""
    x = _ctx(cid)
    hd, dt, c = x.hd, x.dt, x.c
    rng = np.random.default_rng(c.seed + 2 + n_prev)
    eps = float(torch.finfo(dt).eps)
    ks = [t(0.1 * rng.normal(size=x.u.shape), dt) for _ in range(n_prev)]
    cc = [0.1, -0.05, 0.02, 0.07, -0.03, 0.04][:n_prev]
    ec = [0.01, -0.02, 0.03, 0.04, -0.015, 0.025, 0.05][:n_prev] + [0.04]
    y = torch.empty_like(x.ut)
    sumsq = torch.zeros(1, dtype=torch.float64, device=device())
    du = hd.rhs_stage(x.pt, x.ut, ks, cc, y_out=y, error=(ec, 1e-6, 1e-3, sumsq))
    assert _last(hd) == c.rhs_stage_path
    y_ref = x.ut.clone()
    for cj, k in zip(cc, ks):
        y_ref = y_ref + cj * k
    assert (y - y_ref).abs().max().item() <= (1.5 * n_prev + 0.5) * eps * max(1.0, y_ref.abs().max().item())
    lks = [t(rng.normal(size=x.u.shape), dt) for _ in range(n_adj)]
    lc = [0.3, -0.2, 0.15, -0.1, 0.05][:n_adj]
    ls = torch.empty_like(x.ut)
    lamJ, dp = hd.vjp_stage(x.pt, x.ut, ks, cc, x.lt, lks, lc, lam_out=ls)
    assert _last(hd) == c.vjp_path
    ls_ref = x.lt.clone()
    for cj, k in zip(lc, lks):
        ls_ref = ls_ref + cj * k
    assert (ls - ls_ref).abs().max().item() <= (1.5 * n_adj + 0.5) * eps * max(1.0, ls_ref.abs().max().item())
    du_ref = hd.rhs(x.pt, y)
    lamJ_ref, dp_ref = hd.vjp(x.pt, y, ls)
    ys, xs, ps = LC.chain_error_scale(x.specs, x.p, _f64(y), _f64(ls))
    if c.rhs_stage_path == CC.EVAL_PER_LAYER and c.rhs_path == CC.EVAL_PER_LAYER:
        assert torch.equal(du, du_ref)
    else:
        assert_close(du, _f64(du_ref), ys, x.rtol, "stage du")
    if not c.cls.vjp:
        assert torch.equal(lamJ, lamJ_ref) and torch.equal(dp, dp_ref)
    else:
        assert_close(lamJ, _f64(lamJ_ref), xs, x.rtol, "stage xbar")
        assert_close(dp, _f64(dp_ref), ps, x.rtol, "stage pbar")
    assert_close(du, O.chain_fwd(x.specs, x.p, _f64(y)), ys, x.rtol, "stage du against the oracle")
    rJ, rdp = O.chain_vjp(x.specs, x.p, _f64(y), _f64(ls))
    assert_close(lamJ, rJ, xs, x.rtol, "stage xbar against the oracle")
    assert_close(dp, rdp, ps, x.rtol, "stage pbar against the oracle")
    e = ec[-1] * du.double()
    for ej, k in zip(ec, ks):
        e = e + ej * k.double()
    sk = 1e-6 + 1e-3 * torch.maximum(x.ut.double().abs(), y.double().abs())
    want = ((e / sk) ** 2).sum().item()
    assert abs(sumsq.item() - want) <= 1e-12 * want


def _step_inputs(x):
    """u0 inside the grid limits and parameters of a third the Glorot size (a tame right-hand side), seeded."""
    rng = np.random.default_rng(x.c.seed + 3)
    lo, hi = x.c.row.lims
    return t(rng.uniform(lo, hi, x.u.shape), x.dt), t(x.p / 3.0, x.dt)


@pytest.mark.parametrize("cid", STEPS)
def test_fused_forward_step_equals_the_stage_launches(cid):
    """kd_chain_step_kernel: a fixed-step host-loop solve of 3 steps with KANODE_OPT_FUSED_STEP 1 (one launch per
    step) against 0 (six kanode_rhs_stage launches per step).  Both run chain_forward on the same stage inputs in the
    same fma order: bitwise equal.  last_eval names the step kernel / the one-launch stage kernel."""
    x = _ctx(cid)
    hd = x.hd
    u0, p = _step_inputs(x)
    opts = kanode.Tsit5Options(adaptive=False, dt=0.05).to_c()
    saveat = [0.0, 0.05, 0.1, 0.15]
    out = {}
    for fused in (1, 0):
        with hd.options(fused_step=fused):
            us, stats, _ = hd.solve_tsit5(p, u0, 0.0, 0.15, saveat, opts)
            torch.cuda.synchronize()
            out[fused] = (us, stats, _last(hd))
    assert out[1][1]["naccept"] == out[0][1]["naccept"] == 3
    assert out[1][2] == CC.EVAL_CHAIN_STEP and out[0][2] == CC.EVAL_CHAIN_KERNEL
    assert torch.isfinite(out[1][0]).all()
    assert torch.equal(out[1][0], out[0][0])


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("cid", STEPS)
def test_fused_adjoint_step_equals_the_stage_launches(cid, adaptive):
    """kd_chain_vjp_step_kernel: the host-loop InterpolatingAdjoint with one launch per step against six
    kanode_vjp_stage launches and their reductions.  Same per-column arithmetic, same blocks, same reduction order:
    du0 and dp bitwise equal, with the same step sequence.  last_eval names the adjoint step kernel / the one-launch
    adjoint stage kernel; where the step kernel's seven gradient rows per group do not fit in LDS
    (chain_cases.ADJ_STEP: ss_g7 and tanh_g10 in fp64) FUSED_STEP = 1 runs the stage kernel as well, and says so."""
    x = _ctx(cid)
    fits = CC.ADJ_STEP[x.c.row.name][0 if x.c.dtype == "f64" else 1]
    u0, p0 = _step_inputs(x)
    rhs = kanode.ChainRHS(cfgs_from_specs(x.specs), dtype=x.dt, device=device())
    ts = [0.1 * i for i in range(6)]
    w = t(np.random.default_rng(x.c.seed + 4).normal(size=(len(ts),) + x.u.shape), x.dt)
    opt = kanode.Tsit5Options() if adaptive else kanode.Tsit5Options(adaptive=False, dt=0.05)
    res = {}
    for fused in (1, 0):
        with rhs.hd.options(fused_step=fused):
            p = p0.clone().requires_grad_(True)
            x0 = u0.clone().requires_grad_(True)
            sol = kanode.solve(rhs, x0, (0.0, 0.5), p, ts, opt, sensealg="interpolating_adjoint")
            gp, gu = torch.autograd.grad((sol.u * w).sum(), [p, x0])
            torch.cuda.synchronize()
            res[fused] = (gp, gu, sol.stats, _last(rhs.hd))
    (g1, u1, s1, e1), (g0, u0_, s0, e0) = res[1], res[0]
    assert e1 == (CC.EVAL_CHAIN_ADJ_STEP if fits else CC.EVAL_CHAIN_KERNEL) and e0 == CC.EVAL_CHAIN_KERNEL
    assert s1["adjoint"]["naccept"] == s0["adjoint"]["naccept"] and s1["adjoint"]["nreject"] == s0["adjoint"]["nreject"]
    assert torch.isfinite(g1).all() and torch.isfinite(u1).all()
    assert torch.equal(g1, g0)
    assert torch.equal(u1, u0_)
