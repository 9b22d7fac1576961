"""The device-resident Fisher-KPP training loop on the forward-mode gradient (kanode_train_forward_tsit5,
Trainer.run; fk_small_train_kernel): K whole iterations of Fisher-KPP_Source.jl:194-213 in one launch.  Every
iteration is checked on its own through the per-iteration records (p_before, grad, counts), so nothing compounds
through Adam: against the one-launch path (kanode_forward_sensitivity_tsit5 + the host contraction), kanode_adam_step
and kanode.solve.

The bars.  The loop runs the device functions of the one-launch path on the same tables, so the solves are bitwise
equal and no step decision can differ (the counts are equal); gradient and loss then differ by the summation order
alone.  With N = n_save·nx·B terms per sum, each ordering of N rounded products lies within γ_{N+1} of the exact sum:
    |g_k - g_k^ref| <= 4·N·2⁻⁵³·Σ_{j,i}|dl_ji·S_jki|        (the 4 covers both orderings and second-order terms)
    |L - L^ref|     <= 4·N·2⁻⁵³·L                           (non-negative terms: test_gpu_train_loop.py's rule)

With a test problem counts[:, 2:] hold the logged-loss solve's naccept and nreject (there is no adjoint; without one
they are zero), and equal kanode.solve's at every iteration."""
import numpy as np
import pytest
import torch

import bench
import kanode
from kanode import _lib as L
from kanode.adjoint import native_forward_sens
from gpu_util import device, t

pytestmark = pytest.mark.gpu

TSPAN, SAVEAT, ETA = (0.0, 2.0), [0.5 * i for i in range(5)], 1e-2
OPTS = {"fixed": dict(adaptive=False, dt=0.01), "default": dict()}
# case: nx, B, G, normalizer
CASES = {"a": (26, 1, 10, "softsign"), "b": (7, 2, 5, "tanh_fast"), "c": (26, 3, 10, "softsign"),
         "d": (65, 1, 10, "softsign")}
ON_DEVICE_TEST = {"a": True, "b": False, "c": True, "d": False}


def problem(case):
    nx, B, G, norm = CASES[case]
    rng = np.random.default_rng(11 + ord(case))
    x = np.arange(nx) / nx
    c = rng.uniform(0.3, 0.7, (B, 1))
    d = np.abs(x[None, :] - c)
    u0 = np.exp(-(np.minimum(d, 1.0 - d) / 0.15) ** 2)             # a smooth periodic bump in [0, 1] per trajectory
    X = rng.uniform(0.0, 1.0, (len(SAVEAT), B, nx))
    p0 = bench.fk_trained_like_params() if G == 10 else rng.normal(0.0, 0.3, G + 1)
    return dict(nx=nx, B=B, G=G, norm=norm, u0=u0, X=X, p0=p0)


def make_rhs(case):
    pr = problem(case)
    kan1 = kanode.Chain(kanode.KDense(1, 1, pr["G"], normalizer=pr["norm"], basis_func="rbf"))
    return kanode.FisherKPPRHS(kan1, nx=pr["nx"], dx=1.0 / pr["nx"], D=0.01, dtype=torch.float64, device=device())


def trainer(case, rhs, p=None, opt="default", target=None):
    pr = problem(case)
    return kanode.Trainer(rhs, t(pr["u0"]), TSPAN, SAVEAT, t(pr["X"]) if target is None else target,
                          t(pr["p0"]) if p is None else p.clone(), eta=ETA, solver=kanode.Tsit5Options(**OPTS[opt]))


def state(tr):
    m, v, bp = tr.opt.state[id(tr.p)]
    return tr.p.clone(), m.clone(), v.clone(), list(bp)


_RUNS = {}


def run3(case, opt):
    """run(3, record=True) of one case at one solver setting, computed once and shared (read-only)."""
    if (case, opt) not in _RUNS:
        rhs = make_rhs(case)
        tr = trainer(case, rhs, opt=opt)
        out = tr.run(3, record=True)
        _RUNS[(case, opt)] = (out, state(tr), rhs, tr.last_run)
    return _RUNS[(case, opt)]


@pytest.mark.parametrize("opt", ["fixed", "default"])
@pytest.mark.parametrize("case", list(CASES))
def test_each_iteration_equals_the_one_launch_path(case, opt):
    out, _, rhs, last = run3(case, opt)
    pr = problem(case)
    P, N = pr["G"] + 1, len(SAVEAT) * pr["nx"] * pr["B"]
    assert last == "device_forward"
    assert out["loss"].shape == (3,) and out["grad"].shape == (3, P) and out["counts"].shape == (3, 4)
    assert torch.equal(out["p_before"][0], t(pr["p0"]))
    assert out["counts"][:, 2:].abs().sum().item() == 0
    for it in range(3):
        ref = trainer(case, rhs, out["p_before"][it], opt)
        loss, g, sol = ref.loss_and_grad()
        assert sol.stats["sensealg"] == "forward"
        u, S, _ = native_forward_sens(rhs, ref.u0, TSPAN, ref.p, SAVEAT, ref.solver)
        dl = (u - ref.target).mul_(2.0 / u.numel())
        mag = (S.reshape(len(SAVEAT), P, -1) * dl.reshape(len(SAVEAT), 1, -1)).abs().sum((0, 2))
        bar = 4 * N * 2.0 ** -53 * mag
        gerr = (out["grad"][it] - g).abs()
        lerr = abs(out["loss"][it].item() - float(loss)) / float(loss)
        got = out["counts"][it, :2].tolist()
        print(case, opt, it, got, [sol.stats["naccept"], sol.stats["nreject"]], "grad/bar",
              (gerr / bar).max().item(), "loss", lerr, "bar", 4 * N * 2.0 ** -53)
        assert got == [sol.stats["naccept"], sol.stats["nreject"]]
        assert bool((gerr <= bar).all())
        assert lerr <= 4 * N * 2.0 ** -53


@pytest.mark.parametrize("case", list(CASES))
def test_adam_is_exact(case):
    """kanode_adam_step (FusedAdam.update on clones) fed p_before[it], the moments carried so far and grad[it]
    reproduces p_before[it + 1] and the final p, m, v and running powers, bit for bit (both are adam_entry)."""
    out, (p_end, m_end, v_end, bp_end), _, _ = run3(case, "default")
    opt_ = kanode.FusedAdam(ETA)
    x = out["p_before"][0].clone()
    for it in range(3):
        assert torch.equal(x, out["p_before"][it]), it
        opt_.update(x, out["grad"][it].contiguous())
    m, v, bp = opt_.state[id(x)]
    assert torch.equal(x, p_end) and torch.equal(m, m_end) and torch.equal(v, v_end)
    assert bp == bp_end


@pytest.mark.parametrize("case", ["a", "c"])
def test_state_carries_across_launches(case):
    rhs = make_rhs(case)
    res = []
    for how in ("one", "split", "chunk"):
        tr = trainer(case, rhs)
        if how == "one":
            loss = tr.run(3)["loss"]
        elif how == "split":
            loss = torch.cat([tr.run(2)["loss"], tr.run(1)["loss"]])
        else:
            loss = tr.run(3, chunk=1)["loss"]
        assert tr.last_run == "device_forward"
        p, m, v, bp = state(tr)
        b1, b2 = tr.opt.beta
        e1, e2 = b1, b2
        for _ in range(3):
            e1 *= b1
            e2 *= b2
        assert bp == [e1, e2]
        assert len(tr.history) == 3 and tr.history == loss.tolist()
        res.append((p, m, v, loss))
    for r in res[1:]:
        for a_, b_ in zip(res[0], r):
            assert torch.equal(a_, b_)


@pytest.mark.parametrize("case", ["a", "c"])
def test_logged_loss(case):
    """loss_test[it] is the MSE of the plain solve at p_{it+1} (kanode.solve at p_before[it + 1], the final p for
    the last iteration), its step counts (counts[:, 2:]) are that solve's, and giving the test problem changes no bit
    of loss, grad or p."""
    out0, (p0_end, _, _, _), rhs, _ = run3(case, "default")
    pr = problem(case)
    N = len(SAVEAT) * pr["nx"] * pr["B"]
    assert rhs.hd.train_forward_supported(pr["B"], True)
    tr = trainer(case, rhs)
    out = tr.run(3, test=(TSPAN, SAVEAT, t(pr["X"])), record=True)
    assert tr.last_run == "device_forward" and out["loss_test"].shape == (3,)
    assert torch.equal(tr.p, p0_end) and torch.equal(out["loss"], out0["loss"]) and torch.equal(out["grad"], out0["grad"])
    for it in range(3):
        p_next = out["p_before"][it + 1] if it < 2 else tr.p
        sol = kanode.solve(rhs, t(pr["u0"]), TSPAN, p_next, SAVEAT)
        ref = float(kanode.mse_loss(sol.u, t(pr["X"])))
        err = abs(out["loss_test"][it].item() - ref) / ref
        got = out["counts"][it, 2:].tolist()
        print(case, it, out["loss_test"][it].item(), ref, err, got, [sol.stats["naccept"], sol.stats["nreject"]])
        assert got == [sol.stats["naccept"], sol.stats["nreject"]]
        assert err <= 4 * N * 2.0 ** -53
    assert torch.equal(out["counts"][:, :2], out0["counts"][:, :2])


def test_coverage_and_fallback():
    for case, (nx, B, G, _) in CASES.items():
        rhs = make_rhs(case)
        tr = trainer(case, rhs)
        assert tr.sensealg == "auto" and tr._fast_path()[1] == "forward"        # (turns fsens_wide on for c, d)
        assert rhs.hd.train_forward_supported(B, False), case
        assert rhs.hd.train_forward_supported(B, True) == ON_DEVICE_TEST[case], case
        assert not rhs.hd.train_supported(B)
    # a test problem on a shape without the plain one-workgroup solve: the raw call refuses, run() falls back
    rhs = make_rhs("b")
    pr = problem("b")
    tr = trainer("b", rhs)
    p = tr.p.clone()
    z = torch.zeros_like(p)
    with pytest.raises(L.KanodeError, match="not supported"):
        rhs.hd.train_forward_tsit5(p, z.clone(), z.clone(), t(pr["u0"]), 0.0, 2.0, SAVEAT, t(pr["X"]),
                                   tr.solver.to_c(), ETA, (0.9, 0.999), 1e-8, [0.9, 0.999], 2,
                                   test=(2.0, SAVEAT, t(pr["X"])))
    out = tr.run(2, test=(TSPAN, SAVEAT, t(pr["X"])))
    assert tr.last_run == "host" and out["loss_test"].shape == (2,)
    ref = trainer("b", rhs)
    ls = [ref.step(), ref.step()]
    assert out["loss"].tolist() == ls and torch.equal(tr.p, ref.p)
    # shapes outside the forward rule, and the other loop's handle
    big = kanode.FisherKPPRHS(kanode.Chain(kanode.KDense(1, 1, 10, normalizer="softsign")), nx=256, dx=1.0 / 256,
                              D=0.01, device=device())
    assert not big.hd.train_forward_supported(1, False)
    lv = kanode.ChainRHS(kanode.Chain(kanode.KDense(2, 10, 5), kanode.KDense(10, 2, 5)), dtype=torch.float64,
                         device=device())
    assert not lv.hd.train_forward_supported(1, False) and lv.hd.train_supported(1)


def test_stops_cleanly():
    """maxiters = 3: the Dual solve of iteration 0 stops at maxiters, run raises KanodeError naming it, p, m, v, bp and
    history are untouched, and the next run at the default options succeeds.  (A status path of the kernel.)"""
    rhs = make_rhs("a")
    tr = trainer("a", rhs)
    tr.run(1)
    before, hist = state(tr), list(tr.history)
    good = tr.solver
    tr.solver = kanode.Tsit5Options(maxiters=3)
    with pytest.raises(L.KanodeError, match=r"iteration 0 \(forward_maxiters\)"):
        tr.run(3)
    after = state(tr)
    for a_, b_ in zip(before[:3], after[:3]):
        assert torch.equal(a_, b_)
    assert before[3] == after[3] and tr.history == hist
    tr.solver = good
    assert tr.run(2)["loss"].shape == (2,) and len(tr.history) == 3


def test_it_trains():
    """30 iterations towards the solution at perturbed parameters end below the first loss; afterwards the one-launch
    gradient at tr.p is that of a fresh Trainer there (the loop left the handle's tables and stamps consistent)."""
    rhs = make_rhs("a")
    pr = problem("a")
    with torch.no_grad():
        target = kanode.solve(rhs, t(pr["u0"]), TSPAN, t(pr["p0"] * 1.15 + 0.02), SAVEAT).u.clone()
    tr = trainer("a", rhs, target=target)
    out = tr.run(30)
    assert tr.last_run == "device_forward"
    print(out["loss"][0].item(), out["loss"][-1].item())
    assert out["loss"][-1].item() < out["loss"][0].item()
    l1, g1, _ = tr.loss_and_grad()
    fresh = trainer("a", rhs, tr.p, target=target)
    l2, g2, _ = fresh.loss_and_grad()
    assert float(l1) == float(l2) and torch.equal(g1, g2)
