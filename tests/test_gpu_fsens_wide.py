"""Forward sensitivities for fields of 65 to 128 entries (kan_small.hip fk_small_fsens_kernel with two state entries
per lane, KANODE_OPT_FSENS_WIDE): SciMLSensitivity 7.69 takes ForwardDiffSensitivity wherever length(u0) +
length(p) <= 100, i.e. up to 89 entries at G = 10 and 94 at G = 5, and the one-entry kernel stops at 64.

A  the option gates the coverage;  B  on fields the one-entry kernel covers, the two-entry kernel (fsens_wide = 2)
returns its bits;  C  values AND sensitivities against the C port of the Dual solve, each on its own steps;  D  the
CPU restatement (tests/fsens_restatement.py: oracle RHS / VJP, no HIP inside) replayed on the kernel's recorded
steps, with the reject path (forced first steps) and the fixed step;  E  the host's automatic rule.

Shapes, parameters, comparators and the CPU figures behind the bars: tests/fsens_restatement.py and
tests/test_fsens_wide_cpu.py (which pins the two comparators against each other)."""
import os
import sys

import numpy as np
import pytest
import torch

import kanode
import fsens_restatement as R
from gpu_util import device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _rhs(Nx, G=10, dx=R.DX, D=R.D):
    kan1 = kanode.Chain(kanode.KDense(1, 1, G, normalizer="softsign"))
    return kanode.FisherKPPRHS(kan1, nx=Nx, dx=dx, D=D, device=device())


def _native(pr, opt, wide, rhs=None):
    """The native solve of `pr` with fsens_wide = `wide`: (u, S, stats, ts, dts) as numpy / dict."""
    rhs = rhs or _rhs(pr["Nx"], pr["G"], pr["dx"], pr["D"])
    rhs.hd.set_option("fsens_wide", wide)
    dev = device()
    p, u0 = torch.as_tensor(pr["p"], device=dev), torch.as_tensor(pr["u0"], device=dev)
    u, S, st = rhs.hd.forward_sensitivity_tsit5(p, u0, 0.0, pr["T"], pr["saveat"], opt.to_c())
    ts, dts = rhs.hd.forward_sensitivity_step_sizes()
    assert len(dts) == st["naccept"]
    return u, S, st, ts, dts


def _reference_problem(name):
    """The reference's source problems (26 x 1 Fisher-KPP, 41 x 1 Allen-Cahn) in fsens_restatement's layout."""
    import anchors
    src = anchors.source_problem(name)
    rng = np.random.default_rng(3)
    p = R.params(10)
    if name == "ac":   # (a random KAN of its size, as tests/test_gpu_fsens.py draws it)
        rng.normal(0.0, 0.05, 11)
        p = rng.normal(0.0, 0.5, 11)
    return dict(Nx=src["nx"], B=1, G=10, P=11, D=src["D"], dx=src["dx"], T=src["tspan"][1], tspan=src["tspan"],
                saveat=list(src["saveat"]), u0=src["u0"][None, :].copy(), p=p,
                spec=R.O.LayerSpec(1, 1, 10, "softsign"))


# ---- A ---------------------------------------------------------------------------------------------------------

def test_option_gates_the_coverage():
    rhs = _rhs(26)
    assert rhs.hd.get_option("fsens_wide") == 0
    assert rhs.hd.forward_sensitivity_supported(2) and not rhs.hd.forward_sensitivity_supported(3)
    for Nx, B, G in R.SHAPES:
        h = _rhs(Nx, G).hd
        assert not h.forward_sensitivity_supported(B), (Nx, B)
        h.set_option("fsens_wide", 1)
        assert h.get_option("fsens_wide") == 1
        assert h.forward_sensitivity_supported(B), (Nx, B)
    rhs.hd.set_option("fsens_wide", 1)
    assert not rhs.hd.forward_sensitivity_supported(5)            # 130 entries
    for nx in (129, 256):
        h = _rhs(nx).hd
        h.set_option("fsens_wide", 1)
        assert not h.forward_sensitivity_supported(1)
    for v in (2, 0, 1):
        rhs.hd.set_option("fsens_wide", v)
        assert rhs.hd.get_option("fsens_wide") == v
    with pytest.raises(kanode.KanodeError):
        rhs.hd.set_option("fsens_wide", 3)
    with pytest.raises(kanode.KanodeError):
        rhs.hd.set_option("fsens_wide", -1)
    assert rhs.hd.get_option("fsens_wide") == 1
    # the uncovered-shape message names both limits
    big = _rhs(256)
    dev = device()
    with pytest.raises(kanode.KanodeError, match=r"forward sensitivities:.*<= 64 \(128 with KANODE_OPT_FSENS_WIDE\)"):
        big.hd.forward_sensitivity_tsit5(torch.zeros(11, dtype=torch.float64, device=dev),
                                         torch.zeros((1, 256), dtype=torch.float64, device=dev), 0.0, 1.0, [0.0, 1.0],
                                         kanode.Tsit5Options().to_c())


# ---- B ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["fk", "ac", "13x4"])
def test_two_entry_kernel_returns_the_one_entry_kernels_bits(case):
    """With an empty upper half every per-entry statement and every sum of the two-entry kernel is the one-entry
    kernel's: the reference Fisher-KPP problem (26 x 1, T = 5, default tolerances, table path), the Allen-Cahn one
    (41 x 1, odd: formula path) and four trajectories of 13 points."""
    pr = R.problem(13, 4, 10) if case == "13x4" else _reference_problem(case)
    rhs = _rhs(pr["Nx"], 10, pr["dx"], pr["D"])
    opt = kanode.Tsit5Options()
    u1, S1, st1, ts1, dts1 = _native(pr, opt, 0, rhs)
    u2, S2, st2, ts2, dts2 = _native(pr, opt, 2, rhs)
    assert st1 == st2 and st1["naccept"] > 0
    assert torch.equal(u1, u2) and torch.equal(S1, S2)
    assert np.array_equal(ts1, ts2) and np.array_equal(dts1, dts2)
    assert float(S1.abs().max()) > 0.0


# ---- C ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tol,ubar,sbar", [(1e-3, 1e-6, 1e-6), (1e-6, 1e-9, 1e-8)])
@pytest.mark.parametrize("i", range(len(R.SHAPES)))
def test_wide_kernel_matches_c_port_on_own_steps(i, tol, ubar, sbar):
    """Values and every S_k against oracle.fk_fsens_solve, each solver on its own step sequence: equal accepted /
    rejected counts; u within ubar·max(1, max|u|), S_k within sbar of its own scale.  The 1e-3 bar is
    tests/test_gpu_fsens.py's own-steps bar (>= 15x the CPU figure between the C port and the restatement, 6.6e-8);
    the 1e-6 bars are two orders over the CPU figures (1e-12, 6e-11)."""
    pr = R.problem(*R.SHAPES[i])
    uc, Sc, stc = R.c_port(pr, tol)
    u, S, st, _, _ = _native(pr, kanode.Tsit5Options(abstol=tol * 1e-3, reltol=tol), 1)
    eu, es = R.worst(u.cpu().numpy(), S.cpu().numpy(), uc, Sc)
    print(f"C {R.SHAPES[i]} tol {tol}: native {st} C port {stc} u {eu:.3g} S {es:.3g}")
    assert (st["naccept"], st["nreject"]) == (stc["naccept"], stc["nreject"])
    assert eu <= ubar
    assert es <= sbar


# ---- D ---------------------------------------------------------------------------------------------------------

def _replay_check(pr, opt, wide, what):
    """The restatement on the kernel's recorded steps: u within 1e-10 of its scale, each S_k within 1e-9 of its own
    (tests/test_gpu_fsens.py's replay bars: per entry the arithmetic is the same).  Measured on the MI355X: at most
    1.0e-12 / 6.9e-12, except (89, 1) at the default tolerances (eight steps at the stability limit): 8.4e-11 / 3.5e-10."""
    u, S, st, ts, dts = _native(pr, opt, wide)
    ur, Sr, na, _ = R.restate(pr, opt, replay=dts)
    assert na == st["naccept"]
    eu, es = R.worst(u.cpu().numpy(), S.cpu().numpy(), ur, Sr)
    print(f"D {what}: native {st} u {eu:.3g} S {es:.3g}")
    assert eu <= 1e-10
    assert es <= 1e-9
    return st


@pytest.mark.parametrize("i", range(len(R.SHAPES)))
def test_wide_kernel_replayed_by_the_cpu_restatement(i):
    pr = R.problem(*R.SHAPES[i])
    _replay_check(pr, kanode.Tsit5Options(), 1, f"{R.SHAPES[i]}")


@pytest.mark.parametrize("Nx,B,G,dt", R.FORCED)
def test_wide_kernel_reject_path_replayed(Nx, B, G, dt):
    """A forced first step the controller rejects (the restatement rejects 2, 3 and 2 steps on the CPU)."""
    pr = R.problem(Nx, B, G)
    st = _replay_check(pr, kanode.Tsit5Options(dt=dt), 1, f"({Nx}, {B}) first step {dt}")
    assert st["nreject"] >= 1


@pytest.mark.parametrize("Nx,B", [(26, 3), (89, 1)])
def test_wide_kernel_fixed_step_replayed(Nx, B):
    pr = R.problem(Nx, B, 10)
    st = _replay_check(pr, kanode.Tsit5Options(adaptive=False, dt=0.05), 1, f"({Nx}, {B}) fixed step")
    assert st["naccept"] == 20 and st["nreject"] == 0


def test_one_entry_kernel_fixed_step_replayed():
    """The fixed step of the one-entry kernel on the reference 26 x 1 problem (default handle): its first two
    evaluations now alternate the exchange slots."""
    pr = _reference_problem("fk")
    st = _replay_check(pr, kanode.Tsit5Options(adaptive=False, dt=0.05), 0, "reference 26 x 1 fixed step")
    assert st["naccept"] == 100 and st["nreject"] == 0


# ---- E ---------------------------------------------------------------------------------------------------------

def _trainer(Nx, B):
    pr = R.problem(Nx, B, 10)
    dev = device()
    rhs = _rhs(Nx)
    p, u0 = torch.as_tensor(pr["p"], device=dev), torch.as_tensor(pr["u0"], device=dev)
    X = torch.as_tensor(np.random.default_rng(4).uniform(0.0, 1.0, (len(pr["saveat"]), B, Nx)), device=dev)
    return pr, rhs, p, u0, X, kanode.Trainer(rhs, u0, pr["tspan"], pr["saveat"], X, p, eta=1e-2)


@pytest.mark.parametrize("Nx,B", [(26, 3), (89, 1)])
def test_trainer_takes_forward_mode_where_the_reference_does(Nx, B):
    """length(u0) + length(p) = 89 and 100 <= 100: forward mode, and the gradient of solve(sensealg="forward") +
    autograd."""
    pr, rhs, p, u0, X, tr = _trainer(Nx, B)
    assert tr.sensealg == "auto" and rhs.hd.get_option("fsens_wide") == 0
    loss, g, sol = tr.loss_and_grad()
    assert sol.stats.get("sensealg") == "forward"
    assert rhs.hd.get_option("fsens_wide") == 1
    pg = p.clone().requires_grad_(True)
    s2 = kanode.solve(rhs, u0, pr["tspan"], pg, pr["saveat"], kanode.Tsit5Options(), sensealg="forward")
    (g2,) = torch.autograd.grad(((s2.u - X) ** 2).mean(), [pg])
    assert g.abs().max().item() > 0.0
    assert (g - g2).abs().max().item() <= 1e-13 * g.abs().max().item()


def test_trainer_takes_the_adjoint_past_the_rule():
    """90 + 11 = 101 > 100: the InterpolatingAdjoint, and the handle's option stays off."""
    _, rhs, _, _, _, tr = _trainer(90, 1)
    _, _, sol = tr.loss_and_grad()
    assert "sensealg" not in sol.stats and "adjoint" in sol.stats
    assert rhs.hd.get_option("fsens_wide") == 0


def test_auto_with_a_gradient_for_u0_takes_the_adjoint():
    """Forward mode differentiates with respect to p alone: sensealg="auto" then chooses the adjoint instead of
    raising; an explicit "forward" still raises."""
    pr, rhs, p, u0, X, _ = _trainer(26, 3)
    pg, ug = p.clone().requires_grad_(True), u0.clone().requires_grad_(True)
    sol = kanode.solve(rhs, ug, pr["tspan"], pg, pr["saveat"], kanode.Tsit5Options(), sensealg="auto")
    gp, gu = torch.autograd.grad(((sol.u - X) ** 2).mean(), [pg, ug])
    assert "adjoint" in sol.stats and gu.abs().max().item() > 0.0
    ref = kanode.solve(rhs, ug, pr["tspan"], pg, pr["saveat"], kanode.Tsit5Options(),
                       sensealg="interpolating_adjoint")
    rp, ru = torch.autograd.grad(((ref.u - X) ** 2).mean(), [pg, ug])
    assert torch.equal(gp, rp) and torch.equal(gu, ru)
    with pytest.raises(ValueError, match="with respect to p only"):
        kanode.solve(rhs, ug, pr["tspan"], pg, pr["saveat"], kanode.Tsit5Options(), sensealg="forward")
