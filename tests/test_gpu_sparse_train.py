"""The sparsity term of the driver's sparse_on = 1 (loss(p) + reg_loss(p, 5e-4, 0), LV_driver_KANODE.jl:187-201) in
the device-resident Lotka-Volterra loop (kanode_train_tsit5 with kanode_set_l1_penalty; Trainer(sparse_reg=λ).run)
and on the native step (Trainer.step / eval_loss).  The problem, P0, ETA and the option sets are
test_gpu_train_loop.py's; every iteration is checked on its own through the per-iteration records.

Bars.  The regularised loss is mse + λ·A, A = Σ|p_q| over 240 entries: two orderings of the 70 non-negative MSE terms
differ by at most 4·70·2⁻⁵³·mse (that file's rule), two orderings of the 240 terms of A by 4·240·2⁻⁵³·λA, so
    |loss - loss_ref| <= 4·70·2⁻⁵³·mse + 4·240·2⁻⁵³·λ·Σ|p|
The gradient is μ + λ·sgn(p) on both sides, one rounded add of an exact ±λ: that file's GBAR of max|g| holds."""
import numpy as np
import pytest
import torch

import bench
from gpu_util import device, t
from test_gpu_train_loop import ETA, GBAR, OPTS, P0, TS, TS_TEST, U0, X, X_TEST, lv, state

import kanode
from kanode import _lib as L

pytestmark = pytest.mark.gpu

LAM = 5e-4
EPS = 2.0 ** -53


def trainer(rhs, p=None, opt="default", lam=LAM):
    return kanode.Trainer(rhs, t(U0), (0.0, 3.5), TS, t(X), t(P0) if p is None else p.clone(), eta=ETA,
                          solver=kanode.Tsit5Options(**OPTS[opt]), sparse_reg=lam)


_RUNS = {}


def run4(opt):
    """Trainer(sparse_reg=λ).run(4, record=True) at one solver setting, computed once and shared (read-only)."""
    if opt not in _RUNS:
        rhs = lv()
        tr = trainer(rhs, opt=opt)
        out = tr.run(4, record=True)
        _RUNS[opt] = (out, state(tr), rhs, tr.last_run)
    return _RUNS[opt]


def test_the_device_loop_is_taken():
    out, _, rhs, last = run4("default")
    assert last == "device_adjoint"
    assert out["loss"].shape == (4,) and out["grad"].shape == (4, 240) and out["counts"].shape == (4, 4)
    assert torch.equal(out["p_before"][0], t(P0))
    assert rhs.hd.get_l1_penalty() == 0.0           # the call's penalty does not stay on the handle


@pytest.mark.parametrize("opt", ["fixed", "tight", "default"])
def test_each_iteration_matches_the_step_path(opt):
    """A fresh Trainer(sparse_reg=λ) at p_before[it] through loss_and_grad(): equal four counts, gradient within GBAR
    of max|g|, loss within the bar of the module docstring."""
    out, _, rhs, _ = run4(opt)
    for it in range(4):
        pb = out["p_before"][it]
        ref = trainer(rhs, pb, opt)
        loss, g, sol = ref.loss_and_grad()
        assert rhs.hd.get_option("last_adjoint") == L.ADJ_CHAIN_WG
        got = out["counts"][it].tolist()
        want = [sol.stats["naccept"], sol.stats["nreject"], sol.stats["adjoint"]["naccept"],
                sol.stats["adjoint"]["nreject"]]
        mse = float(kanode.mse_loss(sol.u, t(X)))
        pen = LAM * float(pb.abs().sum())
        gerr = ((out["grad"][it] - g).abs().max() / g.abs().max()).item()
        lerr = abs(out["loss"][it].item() - float(loss))
        bar = 4 * 70 * EPS * mse + 4 * 240 * EPS * pen
        print(opt, it, got, want, "grad", gerr, "loss", out["loss"][it].item(), "err", lerr, "bar", bar)
        assert got == want
        assert gerr <= GBAR[opt]
        assert lerr <= bar
        assert out["loss"][it].item() > mse          # the penalty is in the recorded loss


def test_iteration_0_against_the_plain_loop():
    """Iteration 0 from the same P0 with and without the penalty: equal counts (the solves do not see λ), the
    gradient exactly grad_plain + λ·sign(P0), the loss difference within 4·240·2⁻⁵³·λΣ|P0| of λΣ|P0|."""
    out, _, rhs, _ = run4("default")
    plain = trainer(rhs, lam=0.0)
    op = plain.run(1, record=True)
    assert plain.last_run == "device_adjoint"
    p0 = t(P0)
    pen = LAM * float(p0.abs().sum())
    assert out["counts"][0].tolist() == op["counts"][0].tolist()
    want = op["grad"][0] + LAM * torch.sign(p0)
    print("grad diff", (out["grad"][0] - want).abs().max().item())
    assert torch.equal(out["grad"][0], want)
    d = out["loss"][0].item() - op["loss"][0].item()
    print("loss", out["loss"][0].item(), op["loss"][0].item(), "diff - pen", d - pen, "bar", 4 * 240 * EPS * pen)
    assert abs(d - pen) <= 4 * 240 * EPS * pen


@pytest.mark.parametrize("opt", ["fixed", "default"])
def test_adam_is_exact(opt):
    """kanode_adam_step fed p_before[it] and grad[it] (the regularised gradient) reproduces p_before[it + 1] and the
    final p, m, v bit for bit."""
    out, (p_end, m_end, v_end, bp_end), _, _ = run4(opt)
    opt_ = kanode.FusedAdam(ETA)
    x = out["p_before"][0].clone()
    for it in range(4):
        assert torch.equal(x, out["p_before"][it])
        opt_.update(x, out["grad"][it].contiguous())
    m, v, bp = opt_.state[id(x)]
    assert torch.equal(x, p_end) and torch.equal(m, m_end) and torch.equal(v, v_end)
    assert bp == bp_end


def test_state_carries_across_launches():
    """run(3) = run(2); run(1) = run(3, chunk=1), bit for bit."""
    rhs = lv()
    res = []
    for how in ("one", "split", "chunk"):
        tr = trainer(rhs)
        if how == "one":
            loss = tr.run(3)["loss"]
        elif how == "split":
            loss = torch.cat([tr.run(2)["loss"], tr.run(1)["loss"]])
        else:
            loss = tr.run(3, chunk=1)["loss"]
        assert tr.last_run == "device_adjoint"
        p, m, v, bp = state(tr)
        assert len(tr.history) == 3 and tr.history == loss.tolist()
        res.append((p, m, v, loss))
    for other in res[1:]:
        for a_, b_ in zip(res[0], other):
            assert torch.equal(a_, b_)


def test_test_loss_is_the_plain_mse():
    """With a test problem loss_test[it] is the plain MSE of the (0, 14) solve at p_{it+1} (no penalty in it:
    the driver's loss_test), at test_gpu_train_loop.py's bar of 282 terms; giving it changes no training bit."""
    rhs = lv()
    a = trainer(rhs)
    oa = a.run(3)
    tr = trainer(rhs)
    out = tr.run(3, test=((0.0, 14.0), TS_TEST, t(X_TEST)), record=True)
    assert tr.last_run == "device_adjoint"
    assert torch.equal(tr.p, a.p) and torch.equal(out["loss"], oa["loss"])
    for it in range(3):
        p_next = out["p_before"][it + 1] if it < 2 else tr.p
        sol = kanode.solve(rhs, t(U0), (0.0, 14.0), p_next, TS_TEST)
        ref = float(kanode.mse_loss(sol.u, t(X_TEST)))
        err = abs(out["loss_test"][it].item() - ref) / ref
        print(it, out["loss_test"][it].item(), ref, err)
        assert err <= 4 * 282 * EPS


def test_an_exact_zero_stops_the_loop():
    """p0 with one exact zero: reg_loss is NaN there (0·log 0), so the loop stops in iteration 0 before its Adam
    step with loss_not_finite and p, m, v are untouched.  (A status path of the kernel, not a fault.)"""
    rhs = lv()
    p0 = t(P0).clone()
    p0[17] = 0.0
    tr = trainer(rhs, p0)
    assert torch.isnan(tr.loss_and_grad()[0])       # the host formula, on the native step
    with pytest.raises(L.KanodeError, match=r"iteration 0 \(loss_not_finite\)"):
        tr.run(2)
    assert tr.last_run == "device_adjoint"
    p, m, v, bp = state(tr)
    assert torch.equal(p, p0) and not m.any() and not v.any() and bp == [0.9, 0.999]
    assert tr.history == [] and rhs.hd.get_l1_penalty() == 0.0


def test_penalty_validation():
    rhs = lv()
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(L.KanodeError, match="finite and >= 0"):
            rhs.hd.set_l1_penalty(bad)
    assert rhs.hd.get_l1_penalty() == 0.0
    rhs.hd.set_l1_penalty(LAM)
    assert rhs.hd.get_l1_penalty() == LAM
    rhs.hd.set_l1_penalty(0.0)


def _fk():
    rng = np.random.default_rng(5)
    nx = 26
    kan1 = kanode.Chain(kanode.KDense(1, 1, 10, normalizer="softsign", basis_func="rbf"))
    rhs = kanode.FisherKPPRHS(kan1, nx=nx, dx=1.0 / nx, D=0.01, dtype=torch.float64, device=device())
    xg = np.arange(nx) / nx
    d = np.abs(xg[None, :] - 0.5)
    u0 = np.exp(-(np.minimum(d, 1.0 - d) / 0.15) ** 2)
    sv = [0.5 * i for i in range(5)]
    return rhs, t(u0), sv, t(rng.uniform(0.0, 1.0, (5, 1, nx))), t(bench.fk_trained_like_params())


def test_the_fisher_kpp_loop_refuses_the_penalty():
    """kanode_train_forward_tsit5 with a non-zero penalty on the handle: "not supported", nothing launched (p
    untouched); Trainer.run with sparse_reg on that handle takes the host loop and equals two step() calls."""
    rhs, u0, sv, X_, p0 = _fk()
    assert rhs.hd.train_forward_supported(1)
    p = p0.clone()
    oc = kanode.Tsit5Options().to_c()
    rhs.hd.set_l1_penalty(LAM)
    try:
        with pytest.raises(L.KanodeError, match="not supported"):
            rhs.hd.train_forward_tsit5(p, torch.zeros_like(p), torch.zeros_like(p), u0, 0.0, 2.0, sv, X_, oc, 1e-2,
                                       (0.9, 0.999), 1e-8, (0.9, 0.999), 2)
    finally:
        rhs.hd.set_l1_penalty(0.0)
    assert torch.equal(p, p0)
    a = kanode.Trainer(rhs, u0, (0.0, 2.0), sv, X_, p0, eta=1e-2, sparse_reg=LAM)
    b = kanode.Trainer(rhs, u0, (0.0, 2.0), sv, X_, p0, eta=1e-2, sparse_reg=LAM)
    plain = kanode.Trainer(rhs, u0, (0.0, 2.0), sv, X_, p0, eta=1e-2)
    out = a.run(2)
    assert a.last_run == "host"
    ls = [b.step(), b.step()]
    assert torch.equal(a.p, b.p) and out["loss"].tolist() == ls == a.history
    assert plain._native_run_path() == "device_forward"      # (the plain trainer keeps its device loop)


def test_eval_loss_keeps_its_forward_with_sparse_reg():
    """eval_loss() returns the plain MSE and keeps its dense output with sparse_reg set; the following step() takes
    its gradient from it and returns the loss and gradient of a trainer that solved again, bit for bit."""
    rhs = lv()
    a, b, plain = trainer(rhs), trainer(rhs), trainer(rhs, lam=0.0)
    lv_ = a.eval_loss()
    assert a._pre is not None
    assert lv_ == plain.eval_loss()
    la, ga, _ = a.loss_and_grad()
    assert a._pre is None
    lb, gb, _ = b.loss_and_grad()
    assert float(la) == float(lb) and torch.equal(ga, gb)
    assert float(la) > lv_
    assert a.step() == b.step() and torch.equal(a.p, b.p)
