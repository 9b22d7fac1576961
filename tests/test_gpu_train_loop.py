"""The device-resident training loop of one Lotka-Volterra trajectory (kanode_train_tsit5, Trainer.run;
kd_chain_train_lvsp_kernel): K whole iterations of LV_driver_KANODE.jl:279-291 in one launch.  Every iteration is
checked on its own through the per-iteration records (p_before, grad, counts), so nothing compounds through Adam:
against the existing two-launch path (kd_chain_tsit5_kernel + kd_chain_adjoint_lvsp_kernel), the C port
(oracle/cpu_epoch.c) and kanode_adam_step."""
import numpy as np
import pytest
import torch

from gpu_util import device, t
from oracle import oracle as O

import kanode
from kanode import _lib as L

pytestmark = pytest.mark.gpu

TS = [0.1 * i for i in range(35)]
TS_TEST = [0.1 * i for i in range(141)]
SPECS = [O.LayerSpec(2, 10, 5, "tanh_fast"), O.LayerSpec(10, 2, 5, "tanh_fast")]
U0 = np.array([[1.0, 1.0]])
X = np.random.default_rng(2).uniform(0.5, 2.0, (35, 1, 2))
X_TEST = np.random.default_rng(3).uniform(0.5, 2.0, (141, 1, 2))
P0 = kanode.Chain(kanode.KDense(2, 10, 5), kanode.KDense(10, 2, 5)).setup(np.random.default_rng(4))[0].astype(
    np.float64) / 10
ETA = 1e-3
OPTS = {"fixed": dict(adaptive=False, dt=0.01), "tight": dict(abstol=1e-9, reltol=1e-9), "default": dict()}
GBAR = {"fixed": 1e-10, "tight": 1e-10, "default": 1e-9}


def lv(dtype=torch.float64):
    return kanode.ChainRHS(kanode.Chain(kanode.KDense(2, 10, 5), kanode.KDense(10, 2, 5)), dtype=dtype,
                           device=device())


def trainer(rhs, p=None, opt="default"):
    return kanode.Trainer(rhs, t(U0), (0.0, 3.5), TS, t(X), t(P0) if p is None else p.clone(), eta=ETA,
                          solver=kanode.Tsit5Options(**OPTS[opt]))


def state(tr):
    m, v, bp = tr.opt.state[id(tr.p)]
    return tr.p.clone(), m.clone(), v.clone(), list(bp)


_RUNS = {}


def run4(opt):
    """run(4, record=True) at one solver setting, computed once and shared (read-only)."""
    if opt not in _RUNS:
        rhs = lv()
        tr = trainer(rhs, opt=opt)
        _RUNS[opt] = (tr.run(4, record=True), state(tr), rhs)
    return _RUNS[opt]


@pytest.mark.parametrize("opt", ["fixed", "tight", "default"])
def test_each_iteration_matches_the_two_launch_path(opt):
    """For every iteration: a fresh Trainer at p_before[it] through loss_and_grad() (the two-launch path) takes the
    same forward and adjoint step counts, its gradient agrees to 1e-10 of its max (fixed step, 1e-9 tolerances:
    the kernel-vs-kernel bar) / 1e-9 (default tolerances), and its loss to 4·70·2⁻⁵³ relative (two differently
    ordered sums of 70 non-negative terms).  At the default tolerances both sides run the same device functions
    at this p0 (seed 4) and no step decision flipped: the counts are equal."""
    out, _, rhs = run4(opt)
    assert out["loss"].shape == (4,) and out["grad"].shape == (4, 240) and out["counts"].shape == (4, 4)
    for it in range(4):
        ref = trainer(rhs, out["p_before"][it], opt)
        loss, g, sol = ref.loss_and_grad()
        assert rhs.hd.get_option("last_adjoint") == L.ADJ_CHAIN_WG
        got = out["counts"][it].tolist()
        want = [sol.stats["naccept"], sol.stats["nreject"], sol.stats["adjoint"]["naccept"],
                sol.stats["adjoint"]["nreject"]]
        gerr = ((out["grad"][it] - g).abs().max() / g.abs().max()).item()
        lerr = abs(out["loss"][it].item() - float(loss)) / float(loss)
        print(opt, it, got, want, "grad", gerr, "loss", lerr)
        assert got == want
        assert gerr <= GBAR[opt]
        assert lerr <= 4 * 70 * 2.0 ** -53
    assert torch.equal(out["p_before"][0], t(P0))


def test_iteration_0_matches_the_c_port():
    """Iteration 0 against oracle/cpu_epoch.c at the default tolerances: equal counts, gradient within 1e-9 of its
    max, loss within 1e-12 relative (test_lv4096_adjoint_matches_cpu_oracle's bars), and p_before[1] within
    1e-9·eta of the C port's p_new (the C port and kanode.Adam agree to that at this p0: checked here on the CPU
    first, with the C port's own gradient)."""
    lc, gc, pn, st, _ = O.chain_epoch(SPECS, P0.copy(), U0, 3.5, TS, X, eta=ETA)
    pa = torch.as_tensor(P0.copy())
    kanode.Adam(ETA).update(pa, torch.as_tensor(gc))
    assert np.abs(pa.numpy() - pn).max() <= 1e-9 * ETA
    out, _, _ = run4("default")
    assert out["counts"][0].tolist() == [st["naccept"], st["nreject"], st["adjoint_naccept"], st["adjoint_nreject"]]
    assert np.abs(out["grad"][0].cpu().numpy() - gc).max() <= 1e-9 * np.abs(gc).max()
    assert abs(out["loss"][0].item() - lc) <= 1e-12 * lc
    assert np.abs(out["p_before"][1].cpu().numpy() - pn).max() <= 1e-9 * ETA


@pytest.mark.parametrize("opt", ["fixed", "default"])
def test_adam_is_exact(opt):
    """kanode_adam_step (FusedAdam.update on clones) fed p_before[it], the moments carried so far and grad[it]
    reproduces p_before[it + 1], and the final p, m, v, bit for bit: both are the same statement (adam_entry), every
    product, sum and quotient rounded on its own (contraction off in it and around the running powers: with it on,
    1 - βp fused with the product that had advanced βp, and iteration 2's parameters differed in the last bit)."""
    out, (p_end, m_end, v_end, bp_end), _ = run4(opt)
    opt_ = kanode.FusedAdam(ETA)
    x = out["p_before"][0].clone()
    for it in range(4):
        print(opt, it, (x - out["p_before"][it]).abs().max().item())
        assert torch.equal(x, out["p_before"][it])
        opt_.update(x, out["grad"][it].contiguous())
    m, v, bp = opt_.state[id(x)]
    assert torch.equal(x, p_end) and torch.equal(m, m_end) and torch.equal(v, v_end)
    assert bp == bp_end


def test_state_carries_across_launches():
    """run(3) = run(2); run(1) = run(3, chunk=1), bit for bit (the same kernel every way); the optimiser's running
    powers are β³ as Python computes it and history holds the three losses."""
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
        p, m, v, bp = state(tr)
        b = [0.9, 0.999]
        for _ in range(3):
            b[0] *= 0.9
            b[1] *= 0.999
        assert bp == b
        assert len(tr.history) == 3 and tr.history == loss.tolist()
        assert tr._pver == 3 and tr._pre is None
        res.append((p, m, v, loss))
    for other in res[1:]:
        for a_, b_ in zip(res[0], other):
            assert torch.equal(a_, b_)


def test_dense_output_from_lds_and_from_global():
    """The 1e-9 case with the default capacity (dense output staged in LDS) and with KANODE_OPT_FUSED_SOLVE_CAP set
    past what LDS holds (read from global memory): p and grad bitwise equal."""
    rhs = lv()
    a = trainer(rhs, opt="tight")
    oa = a.run(3, record=True)      # (the default capacity is the largest that stages)
    b = trainer(rhs, opt="tight")
    with rhs.hd.options(fused_solve_cap=4096):
        ob = b.run(3, record=True)
    assert torch.equal(a.p, b.p) and torch.equal(oa["grad"], ob["grad"]) and torch.equal(oa["loss"], ob["loss"])
    assert torch.equal(oa["counts"], ob["counts"])


def test_test_loss_solve():
    """loss_test[it] is the MSE of the (0, 14) solve at p_{it+1}: against kanode.solve at p_before[it + 1] (the
    final p for the last iteration), with the loss bar of 282 terms; and giving the test problem changes no bit of
    the training results."""
    rhs = lv()
    plain = trainer(rhs)
    op = plain.run(3)
    assert op["loss_test"] is None
    tr = trainer(rhs)
    out = tr.run(3, test=((0.0, 14.0), TS_TEST, t(X_TEST)), record=True)
    assert torch.equal(tr.p, plain.p) and torch.equal(out["loss"], op["loss"])
    assert out["loss_test"].shape == (3,)
    for it in range(3):
        p_next = out["p_before"][it + 1] if it < 2 else tr.p
        sol = kanode.solve(rhs, t(U0), (0.0, 14.0), p_next, TS_TEST)
        ref = float(kanode.mse_loss(sol.u, t(X_TEST)))
        err = abs(out["loss_test"][it].item() - ref) / ref
        # the step counts of the test solve: the records hold a training forward's, so the same solve is run as one
        # (the test problem as the training problem of a one-iteration run at p_next: the same device code on the
        # same inputs, so its loss is loss_test[it] bit for bit) and its counts are compared with the separate solve's
        as_train = kanode.Trainer(rhs, t(U0), (0.0, 14.0), TS_TEST, t(X_TEST), p_next.clone(), eta=ETA)
        o1 = as_train.run(1, record=True)
        print(it, out["loss_test"][it].item(), ref, err, sol.stats, o1["counts"][0].tolist())
        assert o1["loss"][0].item() == out["loss_test"][it].item()
        assert o1["counts"][0, :2].tolist() == [sol.stats["naccept"], sol.stats["nreject"]]
        assert err <= 4 * 282 * 2.0 ** -53


def test_stops_cleanly():
    """A dense-output capacity of 4 steps at the 1e-9 tolerance: the capacity stop fires in iteration 0, run raises
    KanodeError naming it, p, m, v are untouched, and the next run with the default capacity succeeds.  (A status
    path of the kernel, not a fault.)"""
    rhs = lv()
    tr = trainer(rhs, opt="tight")
    tr.run(1)
    before = state(tr)
    with rhs.hd.options(fused_solve_cap=4):
        with pytest.raises(L.KanodeError, match=r"iteration 0 \(dense_capacity\)"):
            tr.run(3)
    after = state(tr)
    for a_, b_ in zip(before[:3], after[:3]):
        assert torch.equal(a_, b_)
    assert before[3] == after[3] and len(tr.history) == 1
    assert tr.run(3)["loss"].shape == (3,) and len(tr.history) == 4


def test_coverage_and_fallback():
    """train_supported is true for the LV handle at one trajectory only; B = 2, fp32 and a [3,6,3] chain are not
    covered: the raw call raises "not supported", and Trainer.run goes through step() and equals two step() calls
    bit for bit."""
    rhs = lv()
    assert rhs.hd.train_supported(1) and not rhs.hd.train_supported(2)
    rhs32 = lv(torch.float32)
    rhs3 = kanode.ChainRHS(kanode.Chain(kanode.KDense(3, 6, 5), kanode.KDense(6, 3, 5)), device=device())
    assert not rhs32.hd.train_supported(1) and not rhs3.hd.train_supported(1)
    oc = kanode.Tsit5Options().to_c()
    rng = np.random.default_rng(8)
    for f, B, dt in ((rhs, 2, torch.float64), (rhs32, 1, torch.float32), (rhs3, 1, torch.float64)):
        N = f.N
        u0 = t(rng.uniform(0.5, 2.0, (B, N)), dt)
        tg = t(rng.uniform(0.5, 2.0, (35, B, N)), dt)
        p = t(rng.uniform(-0.3, 0.3, f.P), dt)
        with pytest.raises(L.KanodeError, match="not supported"):
            f.hd.train_tsit5(p, torch.zeros_like(p), torch.zeros_like(p), u0, 0.0, 3.5, TS, tg, oc, ETA, (0.9, 0.999),
                             1e-8, (0.9, 0.999), 2)
        a = kanode.Trainer(f, u0, (0.0, 3.5), TS, tg, p, eta=ETA)
        b = kanode.Trainer(f, u0, (0.0, 3.5), TS, tg, p, eta=ETA)
        out = a.run(2)
        ls = [b.step(), b.step()]
        assert torch.equal(a.p, b.p) and out["loss"].tolist() == ls == a.history


def test_it_trains():
    """run(50) from p0 at the default tolerances ends below the first loss (test_lv_training_step_reduces_loss's
    sanity), and the cached forward of eval_loss is not reused after a run."""
    rhs = lv()
    tr = trainer(rhs)
    tr.eval_loss()
    out = tr.run(50)
    assert tr._pre is None and tr._pver == 50
    assert out["loss"][-1].item() < out["loss"][0].item()
    loss, g, _ = tr.loss_and_grad()
    ref = trainer(rhs, tr.p).loss_and_grad()
    assert float(loss) == float(ref[0]) and torch.equal(g, ref[1])
    assert float(loss) < out["loss"][0].item()
