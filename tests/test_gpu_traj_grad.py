"""The gradient of a trajectory ensemble: R initial conditions of one small chain at one p, every trajectory an ODE
of its own with its own forward and adjoint step control, one workgroup each, and the mean of the R rows in a fixed
order (kanode_trajectories_gradient_tsit5; KanodeHandle.trajectories_gradient_tsit5, kanode.trajectories_mse_gradient,
kanode.TrajectoryTrainer).  Workgroup r runs the phases of kd_chain_train_wg_kernel once at batch 1 with the adjoint
on the column-group model, so "equal" here is torch.equal against the two-launch batch-1 path (kd_chain_tsit5_kernel,
then kd_chain_adjoint_kernel) on a second handle of the same chain with chain_wide = 0.

Shapes, data and solver settings are tests/test_gpu_train_wg.py's and tests/test_gpu_trajectories.py's: nine
trajectories from default_rng(21).uniform(0.5, 2.0, (9, N)) over (0, 3.5), p = 3·data(sid)[0] (P0 on the LV handle),
against the target default_rng(5).uniform(0.5, 2, (35, R, N))."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_train_wg as WG
from gpu_util import device, t
from test_gpu_train_loop import P0, lv
from test_gpu_trajectories import SPAN, TS, opts, problem
from test_traj_grad_cpu import chunk_order_mean

import kanode
from kanode import _lib as L
from kanode.adjoint import native_forward_dense, native_mse_gradient
from kanode.handle import _ptr, _stream

pytestmark = pytest.mark.gpu

GBAR = WG.GBAR
_REF_RHS = {}
_CALLS = {}


def target(R, N):
    return t(np.random.default_rng(5).uniform(0.5, 2, (35, R, N)))


def ref_rhs(sid):
    """A second handle of the same chain with chain_wide = 0: its batch-1 adjoint is kd_chain_adjoint_kernel."""
    if sid not in _REF_RHS:
        rhs = lv() if sid == "LV" else WG.make_rhs(sid)
        rhs.hd.set_option("chain_wide", 0)
        _REF_RHS[sid] = rhs
    return _REF_RHS[sid]


def call(sid, opt, R=9, **kw):
    """One device call with every optional output, computed once per case and shared (read-only)."""
    key = (sid, opt, R, tuple(sorted(kw.items())))
    if key not in _CALLS:
        rhs, p, u0 = problem(sid, R=R)
        X = target(R, rhs.hd.N)
        assert rhs.hd.trajectories_gradient_supported()
        loss, dp, info = rhs.hd.trajectories_gradient_tsit5(p, u0, SPAN[0], SPAN[1], TS, X, opts(opt, **kw).to_c(),
                                                            rows=True, du0=True, u_save=True)
        _CALLS[key] = (rhs, p, u0, X, loss, dp, info)
    return _CALLS[key]


def two_launch(rhs, p, u0r, Xr, o):
    """native_mse_gradient's statements at one trajectory, with dL/du0 kept: (loss, dp, du0, u_save, six counts)."""
    u_save, st, dense = native_forward_dense(rhs, u0r, SPAN, p, TS, o)
    try:
        loss = torch.nn.functional.mse_loss(u_save, Xr)
        dl = (u_save - Xr).mul_(2.0 / u_save.numel())
        du0, dp, ast = rhs.hd.adjoint_tsit5(p, dense, dl, o.to_c(), tuple(u0r.shape))
    finally:
        rhs.hd.release_dense(dense)
    return loss, dp, du0, u_save, [st["naccept"], st["nreject"], st["nf"], ast["naccept"], ast["nreject"], ast["nf"]]


def counts(info, r):
    f, a = info["fwd_stats"][r], info["adj_stats"][r]
    return [f["naccept"], f["nreject"], f["nf"], a["naccept"], a["nreject"], a["nf"]]


CASES = ([(s, o) for s in ("S1", "S4", "S5", "S6", "LV") for o in ("fixed", "default")] +
         [("S1", "tight"), ("S4", "tight")])


@pytest.mark.parametrize("sid,opt", CASES, ids=[f"{s}-{o}" for s, o in CASES])
def test_every_row_is_bitwise_the_two_launch_batch_1_gradient(sid, opt):
    """dp_rows[r], du0[r] and the u_save columns torch.equal, the six step counts ==, for every r.  The two-launch
    path forms its MSE in torch (another summation order than the kernel's wave_mse), so loss_rows[r] is held to
    4·n·2⁻⁵³ relative with n = 35·N, check_against_two_launch's bar; the gradient rows stay bitwise."""
    rhs, p, u0, X, loss, dp, info = call(sid, opt)
    ref = ref_rhs(sid)
    o = opts(opt)
    N = rhs.hd.N
    assert info["stop"] == ["ok"] * 9 and info["dp_rows"].shape == (9, rhs.hd.P)
    assert torch.isfinite(info["dp_rows"]).all() and torch.isfinite(info["u_save"]).all()
    for r in range(9):
        Xr = X[:, r:r + 1].contiguous()
        lr, gr, du0r, ur, cr = two_launch(ref, p, u0[r:r + 1].contiguous(), Xr, o)
        assert ref.hd.get_option("last_adjoint") == L.ADJ_CHAIN_WG
        lerr = abs(float(info["loss_rows"][r]) - float(lr)) / float(lr)
        print(sid, opt, r, counts(info, r), cr, "grad", (info["dp_rows"][r] - gr).abs().max().item(), "loss", lerr)
        assert counts(info, r) == cr
        assert torch.equal(info["dp_rows"][r], gr)
        assert torch.equal(info["du0"][r:r + 1], du0r.reshape(1, N))
        assert torch.equal(info["u_save"][:, r:r + 1], ur)
        assert lerr <= 4 * 35 * N * 2.0 ** -53
    # (two_launch is native_mse_gradient with du0 kept)
    l0, g0, _ = native_mse_gradient(ref, u0[0:1].contiguous(), SPAN, p, TS, o, X[:, 0:1].contiguous())
    assert torch.equal(g0, info["dp_rows"][0])
    assert not torch.equal(info["dp_rows"][0], info["dp_rows"][1])


@pytest.mark.parametrize("sid", ["S1", "LV"])
@pytest.mark.parametrize("opt", ["fixed", "default"])
def test_rows_against_the_default_handles_two_launch_path(sid, opt):
    """With chain_wide = 1 the batch-1 path runs the WideModel (S1) / LV-wave adjoint: other summation orders.  Rows
    within GBAR[opt] of the row's max; the step counts equal, or named here where a last-bit difference moves one."""
    rhs, p, u0, X, loss, dp, info = call(sid, opt)
    assert rhs.hd.get_option("chain_wide") == 1
    o = opts(opt)
    moved = []
    for r in range(9):
        lr, gr, sol = native_mse_gradient(rhs, u0[r:r + 1].contiguous(), SPAN, p, TS, o, X[:, r:r + 1].contiguous())
        a = sol.stats["adjoint"]
        cr = [sol.stats["naccept"], sol.stats["nreject"], sol.stats["nf"], a["naccept"], a["nreject"], a["nf"]]
        gerr = ((info["dp_rows"][r] - gr).abs().max() / gr.abs().max()).item()
        print(sid, opt, r, counts(info, r), cr, "grad", gerr)
        assert counts(info, r)[:3] == cr[:3]       # (the forward is the same kernel code on both paths)
        if counts(info, r) != cr:
            moved.append((r, counts(info, r), cr))
            assert all(abs(x - y) <= 1 for x, y in zip(counts(info, r)[3:5], cr[3:5]))
        assert gerr <= GBAR[opt]
    print("adjoint counts moved by a last-bit difference:", moved)
    assert len(moved) <= 2


@pytest.mark.parametrize("R", [1, 9, 64, 65, 1030])
def test_the_reduction_order(R):
    """dp and loss bitwise the numpy restatement of the chunk-of-64 order on the returned rows (1030: 17 chunks, the
    last of 6, more workgroups than CUs); at 1030 not the plain ascending sum's bits."""
    rhs, p, u0, X, loss, dp, info = call("S1", "default", R=R)
    assert info["stop"] == ["ok"] * R
    rows = np.concatenate([info["dp_rows"].cpu().numpy(), info["loss_rows"].cpu().numpy()[:, None]], axis=1)
    want = chunk_order_mean(rows)
    naive = np.zeros(rows.shape[1])
    for r in range(R):
        naive = naive + rows[r]
    naive = naive / R
    got = np.concatenate([dp.cpu().numpy(), [loss]])
    print(R, "vs restated", np.abs(got - want).max(), "vs ascending sum", np.abs(got - naive).max(),
          "vs numpy mean", np.abs(got - rows.mean(0)).max())
    assert np.array_equal(got, want)
    if R == 1030:
        assert not np.array_equal(got, naive)
    # the total is mse_loss over the whole tensor up to summation order
    whole = float(kanode.mse_loss(info["u_save"], X))
    assert abs(loss - whole) <= 4 * X.numel() * 2.0 ** -53 * whole


@pytest.mark.parametrize("sid", ["S1", "S4"])
def test_c_port_anchor_fixed_step(sid):
    """Trajectory 4 at dt = 0.01 against oracle/cpu_epoch.c at B = 1: 350 forward and 350 adjoint steps, gradient
    within 1e-9 of its max, loss within 1e-12 relative (test_iteration_0_matches_the_c_port_fixed_step's bars)."""
    from oracle import oracle as O
    rhs, p, u0, X, loss, dp, info = call(sid, "fixed")
    lc, gc, _, st, _ = O.chain_epoch(WG.specs_of(sid), p.cpu().numpy().copy(), u0[4:5].cpu().numpy(), 3.5, TS,
                                     X[:, 4:5].cpu().numpy(), adaptive=False, dt=0.01)
    gerr = np.abs(info["dp_rows"][4].cpu().numpy() - gc).max() / np.abs(gc).max()
    lerr = abs(float(info["loss_rows"][4]) - lc) / lc
    print(sid, counts(info, 4), st, "grad", gerr, "loss", lerr)
    assert counts(info, 4)[0:2] == [350, 0] and counts(info, 4)[3:5] == [350, 0]
    assert [st["naccept"], st["nreject"], st["adjoint_naccept"], st["adjoint_nreject"]] == [350, 0, 350, 0]
    assert gerr <= 1e-9
    assert lerr <= 1e-12


def test_finite_difference_of_the_total():
    """S1 at the 1e-9 tolerances, R = 9: central differences of the returned total loss along two random unit
    directions (default_rng(7)) with h = 1e-5 against dp·d, to 1e-5 relative: the truncation scale h² plus the
    1e-9-tolerance noise divided by h.  The CPU statement (kanode.solve on OracleChainRHS through autograd, the same
    problem and directions) measures 7.4e-9 and 5.6e-10, below that bar, so the bar stays 1e-5."""
    rhs, p, u0, X, loss, dp, info = call("S1", "tight")
    o = opts("tight").to_c()
    rng = np.random.default_rng(7)
    h = 1e-5
    for k in range(2):
        d = rng.normal(size=p.numel())
        d = t(d / np.linalg.norm(d))
        lp = rhs.hd.trajectories_gradient_tsit5((p + h * d).contiguous(), u0, 0.0, 3.5, TS, X, o)[0]
        lm = rhs.hd.trajectories_gradient_tsit5((p - h * d).contiguous(), u0, 0.0, 3.5, TS, X, o)[0]
        fd, an = (lp - lm) / (2 * h), float(dp @ d)
        print(k, "fd", fd, "dp.d", an, "rel", abs(fd - an) / abs(an))
        assert abs(fd - an) <= 1e-5 * abs(an)


def test_not_the_batched_problem():
    """S1, default tolerances: Trainer at the matrix u0 is ONE ODE with one step size; here the nine forward counts
    differ from each other and the gradient is another one."""
    rhs, p, u0, X, loss, dp, info = call("S1", "default")
    tr = kanode.Trainer(rhs, u0, SPAN, TS, X, p, solver=opts("default"))
    lb, gb, sol = tr.loss_and_grad()
    nacc = [s["naccept"] for s in info["fwd_stats"]]
    print("forward naccept", nacc, "batched", sol.stats["naccept"], "loss", loss, float(lb),
          "grad diff", ((dp - gb).abs().max() / gb.abs().max()).item())
    assert len(set(nacc)) >= 2
    assert dp.shape == gb.shape and not torch.equal(dp, gb)


def scaled_problem():
    """test_trajectories_cpu.py's maxiters construction: rows 1 and 6 scaled by 8 take 3 forward iterations and 40
    adjoint iterations on the CPU statement, the others at least 19 forward and 53 to 73 adjoint iterations."""
    rhs, p, u0 = problem("S1")
    u0 = u0.clone()
    u0[[1, 6]] *= 8.0
    return rhs, p, u0, target(9, 2)


def grad(rhs, p, u0, X, o):
    return rhs.hd.trajectories_gradient_tsit5(p, u0, 0.0, 3.5, TS, X, o.to_c(), rows=True, du0=True, u_save=True)


def check_stopped(info, loss, dp, free, finished):
    for r in range(9):
        if r in finished:
            assert info["stop"][r] == "ok"
            for k in ("dp_rows", "loss_rows", "du0"):
                assert torch.equal(info[k][r], free[k][r]), (k, r)
            assert torch.equal(info["u_save"][:, r], free["u_save"][:, r])
            assert counts(info, r) == counts(free, r)
        else:
            assert info["stop"][r] != "ok"
            assert torch.isnan(info["dp_rows"][r]).all() and torch.isnan(info["loss_rows"][r])
            assert torch.isnan(info["du0"][r]).all()
    assert np.isnan(loss) and torch.isnan(dp).all()


def test_stops_are_per_trajectory():
    """Status paths, not faults, on the scaled S1 problem at the default tolerances.  maxiters bounds the adjoint's
    iterations too, and an adjoint takes at least one step per saveat interval (35 here): at maxiters = 12 rows 1 and
    6 finish their forward solve (3 iterations) and stop in the adjoint, the others stop in the forward solve, so
    every row stops, each with its own reason.  At maxiters = 45 rows 1 and 6 finish (40 adjoint iterations) and the
    others stop in the adjoint (53 or more): the finished rows keep the bits of the unlimited call.  With a dense
    capacity of 4 steps rows 1 and 6 (3 accepted steps) finish and the others stop with dense_capacity.  Then
    TrajectoryTrainer.step() raises and leaves p, m, v as they were, and the next call with the defaults succeeds."""
    rhs, p, u0, X = scaled_problem()
    l_free, dp_free, free = grad(rhs, p, u0, X, opts("default"))
    its = [(counts(free, r)[0] + counts(free, r)[1], counts(free, r)[3] + counts(free, r)[4]) for r in range(9)]
    print("forward / adjoint iterations", its)
    assert free["stop"] == ["ok"] * 9 and np.isfinite(l_free)
    loss, dp, info = grad(rhs, p, u0, X, opts("default", maxiters=12))
    print("maxiters 12", info["stop"])
    assert info["stop"] == ["adjoint_maxiters" if r in (1, 6) else "forward_maxiters" for r in range(9)]
    check_stopped(info, loss, dp, free, ())
    assert "trajectory 0: forward Tsit5: maxiters" in L.lib().kanode_last_error(rhs.hd._h).decode()
    loss, dp, info = grad(rhs, p, u0, X, opts("default", maxiters=45))
    print("maxiters 45", info["stop"])
    assert info["stop"] == ["ok" if r in (1, 6) else "adjoint_maxiters" for r in range(9)]
    check_stopped(info, loss, dp, free, (1, 6))
    with rhs.hd.options(fused_solve_cap=4):
        loss, dp, info = grad(rhs, p, u0, X, opts("default"))
    print("capacity 4", info["stop"])
    assert info["stop"] == ["ok" if r in (1, 6) else "dense_capacity" for r in range(9)]
    check_stopped(info, loss, dp, free, (1, 6))
    tr = kanode.TrajectoryTrainer(rhs, u0, SPAN, TS, X, p, eta=WG.ETA, solver=opts("default"))
    tr.step()
    before = WG.state(tr)
    with rhs.hd.options(fused_solve_cap=4):
        with pytest.raises(L.KanodeError, match=r"trajectory 0 stopped \(dense_capacity\)"):
            tr.step()
    after = WG.state(tr)
    for a_, b_ in zip(before[:3], after[:3]):
        assert torch.equal(a_, b_)
    assert before[3] == after[3] and len(tr.history) == 1
    tr.step()
    assert len(tr.history) == 2 and tr.last_info["stop"] == ["ok"] * 9
    l2, dp2, again = grad(rhs, p, u0, X, opts("default"))
    assert l2 == l_free and torch.equal(dp2, dp_free) and torch.equal(again["dp_rows"], free["dp_rows"])


def test_launch_groups():
    """S1 with a dense capacity of 1024 steps: a trajectory's private block is 116 KB and the 256 MiB buffer holds a
    group of G (a multiple of 64, about 2240) trajectories.  R = G + 64 runs as two launches; rows of both groups equal
    those of a call on just these trajectories, and dp is the restated reduction of all rows."""
    rhs, p, _ = problem("S1")
    o = opts("default")
    with rhs.hd.options(fused_solve_cap=1024):
        G = rhs.hd.trajectories_gradient_group(0.0, 3.5, 35, o.to_c())
        print("group", G)
        assert 64 <= G <= 4096 and G % 64 == 0
        R = G + 64
        u0 = t(np.random.default_rng(21).uniform(0.5, 2.0, (R, 2)))
        X = target(R, 2)
        loss, dp, info = rhs.hd.trajectories_gradient_tsit5(p, u0, 0.0, 3.5, TS, X, o.to_c(), rows=True)
        pick = [0, 5, G - 1, G, G + 63]
        ls, dps, sub = rhs.hd.trajectories_gradient_tsit5(p, u0[pick].contiguous(), 0.0, 3.5, TS,
                                                          X[:, pick].contiguous(), o.to_c(), rows=True)
    assert info["stop"] == ["ok"] * R and sub["stop"] == ["ok"] * 5
    for k, r in enumerate(pick):
        assert torch.equal(info["dp_rows"][r], sub["dp_rows"][k]), r
        assert torch.equal(info["loss_rows"][r], sub["loss_rows"][k]), r
        assert info["fwd_stats"][r] == sub["fwd_stats"][k] and info["adj_stats"][r] == sub["adj_stats"][k]
    rows = np.concatenate([info["dp_rows"].cpu().numpy(), info["loss_rows"].cpu().numpy()[:, None]], axis=1)
    assert np.array_equal(np.concatenate([dp.cpu().numpy(), [loss]]), chunk_order_mean(rows))
    # without the option the capacity is what fits, 1024 here as well: the same group
    assert rhs.hd.trajectories_gradient_group(0.0, 3.5, 35, o.to_c()) == G
    assert rhs.hd.trajectories_gradient_group(0.0, 3.5, 35, opts("fixed").to_c()) > G   # (350 steps: smaller blocks)


def test_trajectory_trainer_records():
    """S1, R = 9, run(3, record=True): grad[it] is trajectories_mse_gradient at p_before[it], bitwise; FusedAdam on
    clones reproduces p_before[it + 1] and the final p; with sparse_reg the loss and gradient are the host formula
    added to the λ = 0 result."""
    rhs, p, u0, X, loss, dp, info = call("S1", "default")
    tr = kanode.TrajectoryTrainer(rhs, u0, SPAN, TS, X, p, eta=WG.ETA, solver=opts("default"))
    out = tr.run(3, record=True)
    assert tr.last_info["path"] == "device" and len(out["loss"]) == 3 and tr.history == out["loss"]
    assert torch.equal(out["p_before"][0], p) and torch.equal(out["grad"][0], dp) and out["loss"][0] == loss
    ad = kanode.FusedAdam(WG.ETA)
    x = out["p_before"][0].clone()
    for it in range(3):
        assert torch.equal(x, out["p_before"][it])
        l, g, inf = kanode.trajectories_mse_gradient(rhs, u0, SPAN, out["p_before"][it], TS, X, opts("default"))
        assert inf["path"] == "device" and torch.equal(g, out["grad"][it]) and l == out["loss"][it]
        ad.update(x, out["grad"][it].contiguous())
    assert torch.equal(x, tr.p)
    m, v, bp = ad.state[id(x)]
    _, m_end, v_end, bp_end = WG.state(tr)
    assert torch.equal(m, m_end) and torch.equal(v, v_end) and bp == bp_end
    reg = kanode.TrajectoryTrainer(rhs, u0, SPAN, TS, X, p, eta=WG.ETA, solver=opts("default"), sparse_reg=5e-4)
    l1, g1, _ = reg.loss_and_grad()
    l0 = torch.as_tensor(loss, dtype=torch.float64, device=device())
    assert torch.equal(l1, l0 + kanode.reg_loss(p, 5e-4, 0.0)) and torch.equal(g1, dp + 5e-4 * torch.sign(p))
    pred = tr.predict()
    assert pred.path == "device" and pred.u.shape == (35, 9, 2)


def test_trajectory_trainer_trains_lv():
    """LV [2,10,2], 16 initial conditions, targets generated by solve_trajectories at the trained parameters of
    tests/golden/lv_trained_p_seed1.npy: 30 iterations from P0 end below the first loss."""
    import os
    from conftest import ROOT
    rhs = lv()
    u0 = t(np.random.default_rng(21).uniform(0.5, 2.0, (16, 2)))
    pt = t(np.load(os.path.join(ROOT, "tests", "golden", "lv_trained_p_seed1.npy")).astype(np.float64))
    X = kanode.solve_trajectories(rhs, u0, SPAN, pt, TS).u
    assert torch.isfinite(X).all()
    tr = kanode.TrajectoryTrainer(rhs, u0, SPAN, TS, X, t(P0), eta=WG.ETA)
    out = tr.run(30)
    print("loss", out["loss"][0], "->", out["loss"][-1])
    assert tr.last_info["path"] == "device"
    assert all(np.isfinite(out["loss"])) and out["loss"][-1] < out["loss"][0]


def raw_call(hd, p, u0, X, R, n_save=35):
    """The C entry with sentinel-filled outputs: (status, outputs)."""
    P, N = hd.P, hd.N
    dt = p.dtype
    dp = torch.full((P,), 7.0, dtype=dt, device=p.device)
    rows = torch.full((max(R, 1), P), 7.0, dtype=dt, device=p.device)
    lrows = torch.full((max(R, 1),), 7.0, dtype=dt, device=p.device)
    loss = C.c_double(7.0)
    n = max(R, 1)
    fst, ast, stop = (L.SolveStatsC * n)(), (L.SolveStatsC * n)(), (C.c_int32 * n)(*([7] * n))
    sv = (C.c_double * n_save)(*TS[:n_save])
    o = kanode.Tsit5Options().to_c()
    st = L.lib().kanode_trajectories_gradient_tsit5(hd._h, _ptr(p), _ptr(u0), R, 0.0, 3.5, sv, n_save, _ptr(X),
                                                    C.byref(o), C.byref(loss), _ptr(dp), _ptr(rows), _ptr(lrows), None,
                                                    None, fst, ast, stop, _stream(hd.device))
    torch.cuda.synchronize()
    return st, (loss.value, dp, rows, lrows, list(stop))


def untouched(out):
    loss, dp, rows, lrows, stop = out
    return loss == 7.0 and bool((dp == 7).all()) and bool((rows == 7).all()) and bool((lrows == 7).all()) and \
        all(s == 7 for s in stop)


def test_refusals():
    """fp32, the Fisher-KPP field and a [2,20,2] chain: the raw call returns KANODE_ERR_UNSUPPORTED with the outputs
    untouched, and kanode.trajectories_mse_gradient takes its host path; n_traj = 0 and 65537 are invalid."""
    rhs32, p32, u32 = problem("S6", torch.float32, R=2)
    wide = kanode.ChainRHS(kanode.Chain(kanode.KDense(2, 20, 5), kanode.KDense(20, 2, 5)), dtype=torch.float64,
                           device=device())
    fk = kanode.FisherKPPRHS(kanode.Chain(kanode.KDense(1, 1, 5, normalizer="softsign")), nx=26, dx=1.0 / 25, D=0.01,
                             device=device())
    rng = np.random.default_rng(9)
    cases = [("fp32", rhs32, p32, u32, torch.float32),
             ("wide", wide, t(rng.uniform(-0.3, 0.3, wide.hd.P)), t(rng.uniform(0.5, 2.0, (2, 2))), torch.float64),
             ("fk", fk, t(rng.uniform(-0.3, 0.3, fk.hd.P)), t(rng.uniform(0.1, 0.9, (2, 26))), torch.float64)]
    for name, rhs, p, u0, dt in cases:
        hd = rhs.hd
        X = t(np.random.default_rng(5).uniform(0.5, 2, (35, 2, hd.N)), dt)
        assert not hd.trajectories_gradient_supported(), name
        assert hd.trajectories_gradient_group(0.0, 3.5, 35, kanode.Tsit5Options().to_c()) == 0
        st, out = raw_call(hd, p, u0, X, 2)
        print(name, st, L.lib().kanode_last_error(hd._h).decode()[:80])
        assert st == L.ERR_UNSUPPORTED and untouched(out), name
        with pytest.raises(L.KanodeError, match="not supported"):
            hd.trajectories_gradient_tsit5(p, u0, 0.0, 3.5, TS, X, kanode.Tsit5Options().to_c())
        span, ts = ((0.0, 0.3), [0.1, 0.2, 0.3]) if name == "fk" else (SPAN, TS)
        Xs = X[:len(ts)].contiguous()
        loss, dp, info = kanode.trajectories_mse_gradient(rhs, u0, span, p, ts, Xs, rows=True)
        assert info["path"] == "host" and info["stop"] == ["ok", "ok"], name
        l0, g0, _ = native_mse_gradient(rhs, u0[0:1].contiguous(), span, p, ts, kanode.Tsit5Options(),
                                        Xs[:, 0:1].contiguous())
        assert torch.equal(info["dp_rows"][0], g0.reshape(-1)) and np.isfinite(loss) and dp.shape == (hd.P,)
        want = (info["dp_rows"][0] + info["dp_rows"][1]) / 2
        assert torch.equal(dp, want)
    rhs, p, u0 = problem("S1")
    X = target(9, 2)
    for R in (0, 65537):
        st, out = raw_call(rhs.hd, p, u0, X, R)
        assert st == L.ERR_INVALID_ARG and untouched(out), R
    # native=False: the host path on a covered handle, through autograd
    loss, dp, info = kanode.trajectories_mse_gradient(rhs, u0[:2].contiguous(), SPAN, p, TS, X[:, :2].contiguous(),
                                                      opts("fixed", dt=0.05), native=False)
    assert info["path"] == "host" and np.isfinite(loss)


def test_the_handles_other_paths_keep_their_bits():
    """solve_tsit5, solve_trajectories_tsit5 and Trainer(device_loop="any").run(2) on the same handle give the same
    bits before and after a gradient call."""
    rhs = WG.make_rhs("S1")
    _, p, u0 = problem("S1")
    X = target(9, 2)
    o = opts("default")

    def others():
        a = rhs.hd.solve_tsit5(p, u0[0:1].contiguous(), 0.0, 3.5, TS, o.to_c())[:2]
        b = rhs.hd.solve_trajectories_tsit5(p, u0, 0.0, 3.5, TS, o.to_c())
        tr = WG.trainer("S1", rhs, device_loop="any")
        out = tr.run(2, record=True)
        assert tr.last_run == "device_adjoint"
        return a, b, (out["loss"], out["grad"], tr.p.clone())

    a0, b0, c0 = others()
    loss, dp, info = rhs.hd.trajectories_gradient_tsit5(p, u0, 0.0, 3.5, TS, X, o.to_c(), rows=True)
    assert info["stop"] == ["ok"] * 9
    a1, b1, c1 = others()
    assert torch.equal(a0[0], a1[0]) and a0[1] == a1[1]
    assert torch.equal(b0[0], b1[0]) and b0[1] == b1[1] and b0[2] == b1[2]
    for x, y in zip(c0, c1):
        assert torch.equal(x, y)
    # and the gradient call itself repeats its bits after them
    loss2, dp2, info2 = rhs.hd.trajectories_gradient_tsit5(p, u0, 0.0, 3.5, TS, X, o.to_c(), rows=True)
    assert loss2 == loss and torch.equal(dp2, dp) and torch.equal(info2["dp_rows"], info["dp_rows"])
