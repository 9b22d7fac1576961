"""The wide-layer and mixed-class chain kernels against the fp64 C oracle, over the case table of
tests/layer_cases.py: every kernel class and class pair kanode_create can form (kanode_abi.cpp:209-223), the three
load-slot instantiations of the wide-in forward, both dtypes, and the normalizer / basis / base-activation variants
the ABI accepts.  The pass criterion is gpu_util.assert_close at the project's two RTOL values, under three scales
of layer_cases.py: the single-layer scale for every layer call against the oracle at exact inputs (tight); the chain
scale for a chain result against the oracle (sound, but it carries the hidden layers' worst-case error and in fp32
cannot tell a wrong λᵀJ of a multi-layer chain from a right one); and, to make up for that, the chain results against
the composition of the layer calls on the device, bitwise where they run the same launches and under
composition_error_scale for the surrogate pair's two-launch pullback (test_layer_cases_cpu.py shows the scales sound
and what each one discriminates).  One handle and one oracle evaluation per record, shared by the tests."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import layer_cases as LC
from gpu_util import RTOL, assert_close, cfgs_from_specs, device, t
from oracle import oracle as O

import kanode

pytestmark = pytest.mark.gpu

BY_ID = {c.id: c for c in LC.CASES}
TDT = {"f64": torch.float64, "f32": torch.float32}
ALL = list(BY_ID)
PAIRS = [c.id for c in LC.CASES if c.is_pair]
# one record per row and dtype at its larger batch (a full 8-column tile and a ragged one; 64 / 65 at the batch edge)
ROW_REPS = [c.id for c in LC.CASES if c.B == max(c.row.batches) and c.variant == "softsign_iqf_exact"]
STAGE_REPS = [c.id for c in LC.CASES if c.B == max(c.row.batches) and c.variant == "tanh_rswaf"
              and c.row.widths[0] == c.row.widths[-1]] + \
             [c.id for c in LC.CASES if c.B == 64 and c.variant == "softsign_rbf_nobase"]


@functools.lru_cache(maxsize=None)
def _ctx(cid):
    c = BY_ID[cid]
    dt = TDT[c.dtype]
    p, u, yb = c.data()
    specs = c.specs()
    hd = kanode.KanodeHandle(cfgs_from_specs(specs), dtype=dt, rhs_kind="chain", device=device())
    y = O.chain_fwd(specs, p, u)
    xb, pb = O.chain_vjp(specs, p, u, yb)
    ys, xs, ps = LC.error_scale(c)
    for a in (p, u, yb, y, xb, pb, ys, xs, ps):
        a.setflags(write=False)
    offs = np.cumsum([0] + [s.param_length() for s in specs])
    return SimpleNamespace(c=c, dt=dt, rtol=RTOL[dt], specs=specs, hd=hd, p=p, u=u, yb=yb, y=y, xb=xb, pb=pb, ys=ys,
                           xs=xs, ps=ps, offs=offs, pt=t(p.copy(), dt), ut=t(u.copy(), dt), lt=t(yb.copy(), dt))


def _f64(x):
    return x.detach().double().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _composition_scale(cid):
    x = _ctx(cid)
    return LC.composition_error_scale(x.specs, x.p, x.u, x.yb)


def _chain_kernel_possible(c):
    """An all-column chain may take the one-launch chain kernels (kd_chain_col_kernel, kd_chain_vjp_stage_kernel)
    where the layer calls take the per-layer column kernels: another summation order, and other hidden bits."""
    return c.n_layers > 1 and all(k == LC.COL for k in c.classes)


@pytest.mark.parametrize("cid", ALL)
def test_rhs_and_vjp_match_the_oracle(cid):
    """rhs, λᵀJ and dp against the oracle under the chain scale (worst case over the hidden layers' errors: loose on x̄
    in fp32, see layer_cases; test_layer_by_layer holds the discriminating chain comparison).  The VJP without λᵀJ
    and without dp equals the full call bitwise: a surrogate pair's dp-only call takes the four launches and equals
    the pair_vjp = 0 call, its λᵀJ-only call the two launches and equals the full two-launch call.  Only the dp-only
    call of an all-column chain, which leaves the one-launch chain kernel, is held to the bound."""
    x = _ctx(cid)
    hd = x.hd
    assert_close(hd.rhs(x.pt, x.ut), x.y, x.ys, x.rtol, "y")
    lamJ, dp = hd.vjp(x.pt, x.ut, x.lt)
    assert_close(lamJ, x.xb, x.xs, x.rtol, "xbar")
    assert_close(dp, x.pb, x.ps, x.rtol, "pbar")
    with hd.options(pair_vjp=0):
        lamJ0, dp0 = hd.vjp(x.pt, x.ut, x.lt)
    if x.c.is_pair:
        _, dp1 = hd.vjp(x.pt, x.ut, x.lt, want_lamJ=False)       # (vjp_t: without λᵀJ the four launches)
        assert torch.equal(dp1, dp0)
        lamJ1, _ = hd.vjp(x.pt, x.ut, x.lt, accumulate_dp=False)
        assert torch.equal(lamJ1, lamJ)
    with hd.options(pair_vjp=0):
        if x.c.is_pair:
            assert_close(lamJ0, x.xb, x.xs, x.rtol, "xbar (pair_vjp = 0)")
            assert_close(dp0, x.pb, x.ps, x.rtol, "pbar (pair_vjp = 0)")
        else:
            assert torch.equal(lamJ0, lamJ) and torch.equal(dp0, dp)     # the option touches pairs only
        _, dp2 = hd.vjp(x.pt, x.ut, x.lt, want_lamJ=False)
        if _chain_kernel_possible(x.c):
            # an all-column chain with N_in == N_out takes the one-launch chain kernel only when λᵀJ is asked
            # for (vjp_t, kanode_eval.cpp:259-266); the dp-only call runs layer by layer, in another summation order
            assert_close(dp2, _f64(dp0), x.ps, x.rtol, "pbar (dp only, all-column chain)")
        else:
            assert torch.equal(dp2, dp0)
        lamJ2, none = hd.vjp(x.pt, x.ut, x.lt, accumulate_dp=False)
        assert none is None and torch.equal(lamJ2, lamJ0)


@pytest.mark.parametrize("cid", ROW_REPS)
def test_dp_accumulates(cid):
    """A second VJP onto a given dp0 gives dp0 + dp to rounding (the bound of dp, and the addition's rounding)."""
    x = _ctx(cid)
    rng = np.random.default_rng(x.c.seed + 1)
    dp0 = rng.normal(size=x.p.shape).astype(x.c.np_dtype()).astype(np.float64)
    _, dp = x.hd.vjp(x.pt, x.ut, x.lt)
    _, dp2 = x.hd.vjp(x.pt, x.ut, x.lt, dp=t(dp0, x.dt))
    eps = float(torch.finfo(x.dt).eps)
    assert_close(dp2, dp0 + _f64(dp), x.rtol * x.ps + 2 * eps * (np.abs(dp0) + np.abs(_f64(dp))), 1.0, "dp0 + dp")


@pytest.mark.parametrize("cid", ALL)
def test_layer_by_layer(cid):
    """kanode_layer_forward / kanode_layer_vjp of every layer against O.layer_fwd / O.layer_vjp at the layer inputs
    and cotangents the GPU itself produced (exact inputs: the single-layer scale), and the chain's rhs / vjp against
    the composition of the layer calls.  That composition is the discriminating chain check: a surrogate pair's rhs
    and four-launch vjp equal it bitwise, and its default two-launch vjp, which sees the same hidden bits and differs
    in the summation order of the wide-out dot products only, is held to composition_error_scale (the single-layer
    scales, layer 1's x̄ rounding carried once through layer 0: a 1 % error of x̄ leaves it).  A mixed-class chain
    runs the very launches of the layer calls and equals them bitwise.  Only an all-column chain, which may take the
    one-launch chain kernels (other hidden bits), is held to the chain scale."""
    x = _ctx(cid)
    hd, specs = x.hd, x.specs
    pl = [x.pt[x.offs[l]:x.offs[l + 1]].contiguous() for l in range(len(specs))]
    pl64 = [x.p[x.offs[l]:x.offs[l + 1]] for l in range(len(specs))]
    hs = [x.ut]
    for l, s in enumerate(specs):
        hs.append(hd.layer_forward(l, pl[l], hs[l]))
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
    if x.c.is_pair:
        assert torch.equal(y, hs[-1])
        with hd.options(pair_vjp=0):
            lamJ, dp = hd.vjp(x.pt, x.ut, x.lt)
        assert torch.equal(lamJ, g) and torch.equal(dp, torch.cat(pbs))
        _, cx, cp = _composition_scale(cid)
        lamJ2, dp2 = hd.vjp(x.pt, x.ut, x.lt)
        assert_close(lamJ2, _f64(g), cx, x.rtol, "two-launch xbar against the layer calls")
        assert_close(dp2, _f64(torch.cat(pbs)), cp, x.rtol, "two-launch pbar against the layer calls")
    elif not _chain_kernel_possible(x.c):
        assert torch.equal(y, hs[-1])
        lamJ, dp = hd.vjp(x.pt, x.ut, x.lt)
        assert torch.equal(lamJ, g) and torch.equal(dp, torch.cat(pbs))
    else:
        assert_close(y, _f64(hs[-1]), x.ys, x.rtol, "rhs against the layer calls")
        lamJ, dp = hd.vjp(x.pt, x.ut, x.lt)
        assert_close(lamJ, _f64(g), x.xs, x.rtol, "xbar against the layer calls")
        assert_close(dp, _f64(torch.cat(pbs)), x.ps, x.rtol, "pbar against the layer calls")


@pytest.mark.parametrize("cid", PAIRS)
def test_pair_vjp_two_launches_against_four(cid):
    """pair_vjp 1 against 0: within composition_error_scale of each other (the two see the same hidden bits), and
    bitwise reproducible on a repeat call (B = 65 is past kPairMaxK: both settings take the four launches)."""
    x = _ctx(cid)
    hd = x.hd
    assert hd.get_option("pair_vjp") == 1
    lamJ1, dp1 = hd.vjp(x.pt, x.ut, x.lt)
    with hd.options(pair_vjp=0):
        lamJ0, dp0 = hd.vjp(x.pt, x.ut, x.lt)
    _, cx, cp = _composition_scale(cid)
    assert_close(lamJ1, _f64(lamJ0), cx, x.rtol, "xbar, 2 against 4 launches")
    assert_close(dp1, _f64(dp0), cp, x.rtol, "pbar, 2 against 4 launches")
    if x.c.B > 64:
        assert torch.equal(lamJ1, lamJ0) and torch.equal(dp1, dp0)
    lamJ1b, dp1b = hd.vjp(x.pt, x.ut, x.lt)
    assert torch.equal(lamJ1b, lamJ1) and torch.equal(dp1b, dp1)


@pytest.mark.parametrize("cid", STAGE_REPS)
def test_stages(cid):
    """kanode_rhs_stage (3 previous stages, y_out, error sum) and kanode_vjp_stage (2 adjoint stages, lam_out) against
    rhs / vjp at the stage inputs they wrote out (which equal torch's combinations to rounding): bitwise for a
    surrogate pair and for a mixed-class chain (the same launches after the combination), within the chain scale for
    an all-column chain (the one-launch kernels); the error sum against torch's to 1e-12 relative."""
    x = _ctx(cid)
    hd, dt = x.hd, x.dt
    rng = np.random.default_rng(x.c.seed + 2)
    eps = float(torch.finfo(dt).eps)
    ks = [t(0.1 * rng.normal(size=x.u.shape), dt) for _ in range(3)]
    c = [0.1, -0.05, 0.02]
    ec = [0.01, -0.02, 0.03, 0.04]
    y = torch.empty_like(x.ut)
    sumsq = torch.zeros(1, dtype=torch.float64, device=device())
    du = hd.rhs_stage(x.pt, x.ut, ks, c, y_out=y, error=(ec, 1e-6, 1e-3, sumsq))
    y_ref = x.ut + c[0] * ks[0] + c[1] * ks[1] + c[2] * ks[2]
    assert (y - y_ref).abs().max().item() <= 4.5 * eps * max(1.0, y_ref.abs().max().item())
    lam = x.lt
    lks = [t(rng.normal(size=x.u.shape), dt) for _ in range(2)]
    lc = [0.3, -0.2]
    ls = torch.empty_like(x.ut)
    lamJ, dp = hd.vjp_stage(x.pt, x.ut, ks, c, lam, lks, lc, lam_out=ls)
    ls_ref = lam + lc[0] * lks[0] + lc[1] * lks[1]
    assert (ls - ls_ref).abs().max().item() <= 4.5 * eps * max(1.0, ls_ref.abs().max().item())
    du_ref = hd.rhs(x.pt, y)
    lamJ_ref, dp_ref = hd.vjp(x.pt, y, ls)
    if not _chain_kernel_possible(x.c):
        assert torch.equal(du, du_ref)
        assert torch.equal(lamJ, lamJ_ref) and torch.equal(dp, dp_ref)
    else:
        ys, xs, ps = LC.chain_error_scale(x.specs, x.p, _f64(y), _f64(ls))
        assert_close(du, _f64(du_ref), ys, x.rtol, "stage du")
        assert_close(lamJ, _f64(lamJ_ref), xs, x.rtol, "stage xbar")
        assert_close(dp, _f64(dp_ref), ps, x.rtol, "stage pbar")
    # and the stage results against the oracle at those inputs
    ys, xs, ps = LC.chain_error_scale(x.specs, x.p, _f64(y), _f64(ls))
    assert_close(du, O.chain_fwd(x.specs, x.p, _f64(y)), ys, x.rtol, "stage du against the oracle")
    rJ, rdp = O.chain_vjp(x.specs, x.p, _f64(y), _f64(ls))
    assert_close(lamJ, rJ, xs, x.rtol, "stage xbar against the oracle")
    assert_close(dp, rdp, ps, x.rtol, "stage pbar against the oracle")
    e = ec[0] * ks[0].double() + ec[1] * ks[1].double() + ec[2] * ks[2].double() + ec[3] * du.double()
    sk = 1e-6 + 1e-3 * torch.maximum(x.ut.double().abs(), y.double().abs())
    want = ((e / sk) ** 2).sum().item()
    assert abs(sumsq.item() - want) <= 1e-12 * want
