"""The device-resident training loop for small chains other than one Lotka-Volterra trajectory
(KANODE_OPT_TRAIN_ANY_CHAIN, Trainer(device_loop="any"); kd_chain_train_wg_kernel): a pruned [2,4,2], a batch, N = 3,
three layers.  As in test_gpu_train_loop.py every iteration is checked on its own through the per-iteration records:
against the two-launch path (kd_chain_tsit5_kernel + the one-workgroup adjoint), the C port (oracle/cpu_epoch.c) and
kanode_adam_step."""
import numpy as np
import pytest
import torch

from gpu_util import device, t
from oracle import oracle as O

import kanode
from kanode import _lib as L

pytestmark = pytest.mark.gpu

TS = [0.1 * i for i in range(35)]
TS_TEST = [0.1 * i for i in range(71)]
ETA = 1e-3
OPTS = {"fixed": dict(adaptive=False, dt=0.01), "tight": dict(abstol=1e-9, reltol=1e-9), "default": dict()}
GBAR = {"fixed": 1e-10, "tight": 1e-10, "default": 1e-9}   # test_gpu_train_loop.py's kernel-vs-kernel bars
# id: (layer widths, normalizer, B): each the smallest shape that reaches its path
SHAPES = {"S1": ([2, 4, 2], "tanh_fast", 1),       # a pruned LV net; WideModel adjoint
          "S2": ([2, 4, 2], "softsign", 3),        # ChainModel, one partly filled wave
          "S3": ([2, 7, 2], "tanh_fast", 16),      # four full waves; block sums across waves
          "S4": ([3, 6, 3], "tanh_fast", 1),       # N = 3: not wide_fits, ChainModel at B = 1
          "S5": ([2, 5, 5, 2], "tanh_fast", 2),    # three layers
          "S6": ([2, 10, 2], "tanh_fast", 2)}      # the ChainShapeLV specialisation with a batch
ALL = sorted(SHAPES)


def chain_of(sid):
    w, norm, _ = SHAPES[sid]
    return kanode.Chain(*[kanode.KDense(i, o, 5, normalizer=norm) for i, o in zip(w, w[1:])])


def specs_of(sid):
    w, norm, _ = SHAPES[sid]
    return [O.LayerSpec(i, o, 5, norm) for i, o in zip(w, w[1:])]


def data(sid):
    """p, u0 (B, N), target (35, B, N) from default_rng(11), in this order."""
    w, _, B = SHAPES[sid]
    rng = np.random.default_rng(11)
    p = rng.uniform(-0.3, 0.3, chain_of(sid).parameterlength())
    u0 = rng.uniform(0.5, 2.0, (B, w[0]))
    X = rng.uniform(0.5, 2.0, (35, B, w[0]))
    return p, u0, X


def make_rhs(sid, dtype=torch.float64):
    return kanode.ChainRHS(chain_of(sid), dtype=dtype, device=device())


def trainer(sid, rhs, p=None, opt="default", **kw):
    p0, u0, X = data(sid)
    return kanode.Trainer(rhs, t(u0), (0.0, 3.5), TS, t(X), t(p0) if p is None else p.clone(), eta=ETA,
                          solver=kanode.Tsit5Options(**OPTS[opt]), **kw)


def state(tr):
    m, v, bp = tr.opt.state[id(tr.p)]
    return tr.p.clone(), m.clone(), v.clone(), list(bp)


_RUNS = {}


def run3(sid, opt):
    """run(3, record=True) with device_loop="any" at one shape and solver setting, computed once and shared
    (read-only)."""
    if (sid, opt) not in _RUNS:
        rhs = make_rhs(sid)
        tr = trainer(sid, rhs, opt=opt, device_loop="any")
        out = tr.run(3, record=True)
        assert tr.last_run == "device_adjoint"
        _RUNS[(sid, opt)] = (out, state(tr), rhs)
    return _RUNS[(sid, opt)]


def check_against_two_launch(sid, opt, out, rhs, **kw):
    _, _, B = SHAPES[sid]
    n = 35 * B * SHAPES[sid][0][0]
    for it in range(out["loss"].shape[0]):
        ref = trainer(sid, rhs, out["p_before"][it], opt, **kw)
        loss, g, sol = ref.loss_and_grad()
        assert rhs.hd.get_option("last_adjoint") == L.ADJ_CHAIN_WG
        got = out["counts"][it].tolist()
        want = [sol.stats["naccept"], sol.stats["nreject"], sol.stats["adjoint"]["naccept"],
                sol.stats["adjoint"]["nreject"]]
        gerr = ((out["grad"][it] - g).abs().max() / g.abs().max()).item()
        lerr = abs(out["loss"][it].item() - float(loss)) / float(loss)
        print(sid, opt, it, got, want, "grad", gerr, "bitwise" if torch.equal(out["grad"][it], g) else "not bitwise",
              "loss", lerr)
        assert got == want
        assert gerr <= GBAR[opt]
        assert lerr <= 4 * n * 2.0 ** -53


@pytest.mark.parametrize("sid,opt", [(s, o) for s in ALL for o in ("fixed", "default")] +
                         [("S1", "tight"), ("S3", "tight")])
def test_each_iteration_matches_the_two_launch_path(sid, opt):
    """For every iteration: a fresh Trainer at p_before[it] through loss_and_grad() (kd_chain_tsit5_kernel + the
    one-workgroup adjoint) takes the same four step counts, its gradient agrees to 1e-10 of its max (fixed, tight)
    / 1e-9 (default), and its loss to 4·n·2⁻⁵³ relative (two differently ordered sums of n = 35·B·N non-negative
    terms)."""
    out, _, rhs = run3(sid, opt)
    P = rhs.hd.P
    assert out["loss"].shape == (3,) and out["grad"].shape == (3, P) and out["counts"].shape == (3, 4)
    check_against_two_launch(sid, opt, out, rhs)
    assert torch.equal(out["p_before"][0], t(data(sid)[0]))


@pytest.mark.parametrize("sid", ["S1", "S3", "S5"])
def test_iteration_0_matches_the_c_port_fixed_step(sid):
    """Iteration 0 at dt = 0.01 against oracle/cpu_epoch.c: 350 forward and 350 adjoint steps, gradient within 1e-9
    of its max, loss within 1e-12 relative, p_before[1] within 1e-9·eta of the C port's p_new
    (test_iteration_0_matches_the_c_port's bars)."""
    p0, u0, X = data(sid)
    lc, gc, pn, st, _ = O.chain_epoch(specs_of(sid), p0.copy(), u0, 3.5, TS, X, adaptive=False, dt=0.01, eta=ETA)
    out, _, _ = run3(sid, "fixed")
    gerr = np.abs(out["grad"][0].cpu().numpy() - gc).max() / np.abs(gc).max()
    perr = np.abs(out["p_before"][1].cpu().numpy() - pn).max()
    print(sid, out["counts"][0].tolist(), st, "grad", gerr, "loss", abs(out["loss"][0].item() - lc) / lc, "p", perr)
    assert out["counts"][0].tolist() == [350, 0, 350, 0]
    assert [st["naccept"], st["nreject"], st["adjoint_naccept"], st["adjoint_nreject"]] == [350, 0, 350, 0]
    assert gerr <= 1e-9
    assert abs(out["loss"][0].item() - lc) <= 1e-12 * lc
    assert perr <= 1e-9 * ETA


@pytest.mark.parametrize("sid", ["S3", "S5"])
def test_adam_is_exact(sid):
    """kanode_adam_step (FusedAdam.update on clones) fed p_before[it], the moments carried so far and grad[it]
    reproduces p_before[it + 1] and the final p, m, v and running powers, bit for bit."""
    out, (p_end, m_end, v_end, bp_end), _ = run3(sid, "default")
    opt_ = kanode.FusedAdam(ETA)
    x = out["p_before"][0].clone()
    for it in range(3):
        print(sid, it, (x - out["p_before"][it]).abs().max().item())
        assert torch.equal(x, out["p_before"][it])
        opt_.update(x, out["grad"][it].contiguous())
    m, v, bp = opt_.state[id(x)]
    assert torch.equal(x, p_end) and torch.equal(m, m_end) and torch.equal(v, v_end)
    assert bp == bp_end


def test_state_carries_across_launches():
    """On S2: run(3) = run(2); run(1) = run(3, chunk=1), bit for bit; the running powers are β³ as Python computes
    it, history holds the three losses and _pver counts them."""
    rhs = make_rhs("S2")
    res = []
    for how in ("one", "split", "chunk"):
        tr = trainer("S2", rhs, device_loop="any")
        if how == "one":
            loss = tr.run(3)["loss"]
        elif how == "split":
            loss = torch.cat([tr.run(2)["loss"], tr.run(1)["loss"]])
        else:
            loss = tr.run(3, chunk=1)["loss"]
        assert tr.last_run == "device_adjoint"
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


def test_l1_term():
    """On S1 with sparse_reg = 5e-4: loss[it] and grad[it] against Trainer(sparse_reg=...).loss_and_grad() at
    p_before[it], at the first test's bars; and sparse_reg = 0 is the run without a penalty, bitwise."""
    rhs = make_rhs("S1")
    tr = trainer("S1", rhs, device_loop="any", sparse_reg=5e-4)
    out = tr.run(3, record=True)
    assert tr.last_run == "device_adjoint"
    check_against_two_launch("S1", "default", out, rhs, sparse_reg=5e-4)
    plain, (p_end, _, _, _), _ = run3("S1", "default")
    assert not torch.equal(out["loss"], plain["loss"])
    zero = trainer("S1", rhs, device_loop="any", sparse_reg=0.0)
    oz = zero.run(3, record=True)
    assert torch.equal(zero.p, p_end) and torch.equal(oz["loss"], plain["loss"]) and torch.equal(oz["grad"], plain["grad"])


def test_test_loss_solve():
    """On S1 with the test problem over (0, 7): loss_test[it] is the MSE of that solve at p_{it+1}, against
    kanode.solve there within 4·142·2⁻⁵³; and giving the test problem changes no bit of p, loss or grad."""
    rhs = make_rhs("S1")
    _, u0, _ = data("S1")
    Xt = np.random.default_rng(12).uniform(0.5, 2.0, (71, 1, 2))
    plain, (p_end, _, _, _), _ = run3("S1", "default")
    tr = trainer("S1", rhs, device_loop="any")
    out = tr.run(3, test=((0.0, 7.0), TS_TEST, t(Xt)), record=True)
    assert tr.last_run == "device_adjoint"
    assert torch.equal(tr.p, p_end) and torch.equal(out["loss"], plain["loss"]) and torch.equal(out["grad"], plain["grad"])
    assert out["loss_test"].shape == (3,)
    for it in range(3):
        p_next = out["p_before"][it + 1] if it < 2 else tr.p
        sol = kanode.solve(rhs, t(u0), (0.0, 7.0), p_next, TS_TEST)
        ref = float(kanode.mse_loss(sol.u, t(Xt)))
        err = abs(out["loss_test"][it].item() - ref) / ref
        print(it, out["loss_test"][it].item(), ref, err)
        assert err <= 4 * 142 * 2.0 ** -53


def test_stops_cleanly():
    """On S2 at the 1e-9 tolerances with a dense-output capacity of 4 steps: the capacity stop fires in iteration
    0, run raises KanodeError naming it, p, m, v are untouched, and the next run with the default capacity succeeds.
    (A status path of the kernel, not a fault.)"""
    rhs = make_rhs("S2")
    tr = trainer("S2", rhs, opt="tight", device_loop="any")
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


@pytest.mark.parametrize("sid", ALL)
def test_gate_with_the_option_off(sid):
    """The option's default is 0: train_supported is false, the raw call raises "not supported", and a default
    Trainer.run goes through step() and equals two step() calls bit for bit."""
    rhs = make_rhs(sid)
    p0, u0, X = data(sid)
    B = SHAPES[sid][2]
    assert rhs.hd.get_option("train_any_chain") == 0 and not rhs.hd.train_supported(B)
    p = t(p0)
    with pytest.raises(L.KanodeError, match="not supported"):
        rhs.hd.train_tsit5(p, torch.zeros_like(p), torch.zeros_like(p), t(u0), 0.0, 3.5, TS, t(X),
                           kanode.Tsit5Options().to_c(), ETA, (0.9, 0.999), 1e-8, (0.9, 0.999), 2)
    a, b = trainer(sid, rhs), trainer(sid, rhs)
    out = a.run(2)
    ls = [b.step(), b.step()]
    assert a.last_run == "host" and rhs.hd.get_option("train_any_chain") == 0
    assert torch.equal(a.p, b.p) and out["loss"].tolist() == ls == a.history


def lv_rhs():
    return kanode.ChainRHS(kanode.Chain(kanode.KDense(2, 10, 5), kanode.KDense(10, 2, 5)), device=device())


def test_gate_with_the_option_on():
    """With the option on train_supported covers S1-S6 and still refuses fp32, B = 17 and a [2,20,2] chain; the LV
    handle at one trajectory keeps its kernel and its bits; an EnsembleTrainer on S1 takes its host path."""
    for sid in ALL:
        rhs = make_rhs(sid)
        rhs.hd.set_option("train_any_chain", 1)
        assert rhs.hd.train_supported(SHAPES[sid][2]), sid
    rhs32 = make_rhs("S1", torch.float32)
    rhs32.hd.set_option("train_any_chain", 1)
    assert not rhs32.hd.train_supported(1)
    rhs1 = make_rhs("S1")
    rhs1.hd.set_option("train_any_chain", 1)
    assert rhs1.hd.train_supported(16) and not rhs1.hd.train_supported(17)
    wide = kanode.ChainRHS(kanode.Chain(kanode.KDense(2, 20, 5), kanode.KDense(20, 2, 5)), device=device())
    wide.hd.set_option("train_any_chain", 1)
    assert not wide.hd.train_supported(1)
    with pytest.raises(L.KanodeError):
        rhs1.hd.set_option("train_any_chain", 2)
    # the LV handle: the same kernel, the same bits
    rng = np.random.default_rng(11)
    p = rng.uniform(-0.3, 0.3, 240)
    u0 = rng.uniform(0.5, 2.0, (1, 2))
    X = rng.uniform(0.5, 2.0, (35, 1, 2))
    res = []
    for on in (0, 1):
        rhs = lv_rhs()
        rhs.hd.set_option("train_any_chain", on)
        assert rhs.hd.train_supported(1)
        tr = kanode.Trainer(rhs, t(u0), (0.0, 3.5), TS, t(X), t(p), eta=ETA)
        out = tr.run(3, record=True)
        assert tr.last_run == "device_adjoint"
        res.append((tr.p.clone(), out["loss"], out["grad"], out["counts"]))
    for a_, b_ in zip(*res):
        assert torch.equal(a_, b_)
    # ensembles stay the LV kernel's
    p0, u0, X = data("S1")
    ens = kanode.EnsembleTrainer(rhs1, t(u0), (0.0, 3.5), TS, t(X), t(np.stack([p0, 0.5 * p0])), eta=ETA)
    ens.run(1)
    assert ens.last_run == "host" and rhs1.hd.get_option("train_any_chain") == 1
    pe = t(np.stack([p0, 0.5 * p0]))
    with pytest.raises(L.KanodeError, match="not supported"):
        rhs1.hd.train_ensemble_tsit5(pe, torch.zeros_like(pe), torch.zeros_like(pe), t(u0), 0.0, 3.5, TS, t(X),
                                     kanode.Tsit5Options().to_c(), [ETA, ETA], (0.9, 0.999), 1e-8,
                                     [(0.9, 0.999)] * 2, 1)


def test_train_prune_keep_training():
    """The reference's three steps (LV_driver_KANODE.jl): train [2,10,2] with the L1 term for 8 iterations, slice
    the hidden layer to four fixed nodes (a fixed keep list: no threshold decides the shape), and keep training the
    [2,4,2] network on the device for 50 iterations: it ends below its first loss, and loss_and_grad() afterwards
    equals a fresh Trainer's at the same p."""
    rng = np.random.default_rng(11)
    chain = kanode.Chain(kanode.KDense(2, 10, 5), kanode.KDense(10, 2, 5))
    p = rng.uniform(-0.3, 0.3, 240)
    u0 = t(rng.uniform(0.5, 2.0, (1, 2)))
    X = t(rng.uniform(0.5, 2.0, (35, 1, 2)))
    rhs = kanode.ChainRHS(chain, device=device())
    tr = kanode.Trainer(rhs, u0, (0.0, 3.5), TS, X, t(p), eta=ETA, sparse_reg=5e-4)
    tr.run(8)
    assert tr.last_run == "device_adjoint"
    small, ps = kanode.prune_params(chain, tr.p, [[0, 3, 5, 8]])
    assert [l.out_dims for l in small.layers] == [4, 2] and ps.shape == (96,)
    rhs_s = kanode.ChainRHS(small, device=device())
    cont = kanode.Trainer(rhs_s, u0, (0.0, 3.5), TS, X, ps, eta=ETA, device_loop="any")
    out = cont.run(50)
    assert cont.last_run == "device_adjoint" and cont._pver == 50
    print(out["loss"][0].item(), out["loss"][-1].item())
    assert out["loss"][-1].item() < out["loss"][0].item()
    loss, g, _ = cont.loss_and_grad()
    ref = kanode.Trainer(rhs_s, u0, (0.0, 3.5), TS, X, cont.p, eta=ETA).loss_and_grad()
    assert float(loss) == float(ref[0]) and torch.equal(g, ref[1])
    assert float(loss) < out["loss"][0].item()
