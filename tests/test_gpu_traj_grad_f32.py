"""The gradient of a trajectory ensemble on an fp32 handle: R initial conditions of one small fp32 chain at one p, every
trajectory an ODE of its own, one workgroup each, and the mean of the R float rows in a fixed order
(kanode_trajectories_gradient_f32_tsit5; KanodeHandle.trajectories_gradient_f32_tsit5,
kanode.trajectories_mse_gradient(f32="device"), kanode.TrajectoryTrainer(f32="device")).  Workgroup r runs
onewg_tsit5<float> and onewg_adjoint<float> on the column-group model once at batch 1, so "equal" here is torch.equal
against the two-launch batch-1 path (kd_chain_tsit5_kernel<float>, then kd_chain_adjoint_kernel<float>) on a second
fp32 handle of the same chain with chain_wide = 0.

Shapes, data and solver settings are tests/test_gpu_traj_grad.py's, cast to float32: nine trajectories from
default_rng(21).uniform(0.5, 2.0, (9, N)) over (0, 3.5), p = 3·data(sid)[0] (P0 on the LV handle), against the target
default_rng(5).uniform(0.5, 2, (35, R, N)).  The 1e-9 tolerances of the fp64 file are left out: they are below float's
resolution."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_train_wg as WG
from gpu_util import device, t
from test_gpu_train_loop import P0, lv
from test_gpu_traj_grad import counts, two_launch
from test_gpu_trajectories import SPAN, TS, opts, problem
from test_traj_grad_f32_cpu import chunk_order_mean_f32

import kanode
from kanode import _lib as L
from kanode.adjoint import combine_trajectory_rows, native_mse_gradient
from kanode.handle import _ptr, _stream

pytestmark = pytest.mark.gpu

F32 = torch.float32
U24 = 2.0 ** -24   # float's unit roundoff
_REF_RHS = {}
_CALLS = {}


def target(R, N):
    return t(np.random.default_rng(5).uniform(0.5, 2, (35, R, N)), F32)


def ref_rhs(sid):
    """A second fp32 handle of the same chain with chain_wide = 0: its batch-1 adjoint is kd_chain_adjoint_kernel."""
    if sid not in _REF_RHS:
        rhs = lv(F32) if sid == "LV" else WG.make_rhs(sid, F32)
        rhs.hd.set_option("chain_wide", 0)
        _REF_RHS[sid] = rhs
    return _REF_RHS[sid]


def call(sid, opt, R=9, **kw):
    """One device call with every optional output, computed once per case and shared (read-only)."""
    key = (sid, opt, R, tuple(sorted(kw.items())))
    if key not in _CALLS:
        rhs, p, u0 = problem(sid, F32, R=R)
        X = target(R, rhs.hd.N)
        assert rhs.hd.trajectories_gradient_f32_supported() and not rhs.hd.trajectories_gradient_supported()
        loss, dp, info = rhs.hd.trajectories_gradient_f32_tsit5(p, u0, SPAN[0], SPAN[1], TS, X, opts(opt, **kw).to_c(),
                                                                rows=True, du0=True, u_save=True)
        assert dp.dtype == F32 and info["dp_rows"].dtype == F32 and info["u_save"].dtype == F32
        _CALLS[key] = (rhs, p, u0, X, loss, dp, info)
    return _CALLS[key]


def rows_of(info):
    return np.concatenate([info["dp_rows"].cpu().numpy(), info["loss_rows"].cpu().numpy()[:, None]], axis=1)


def check_row_against_two_launch(sid, opt, rhs, p, u0, X, info, r):
    ref = ref_rhs(sid)
    N = rhs.hd.N
    Xr = X[:, r:r + 1].contiguous()
    lr, gr, du0r, ur, cr = two_launch(ref, p, u0[r:r + 1].contiguous(), Xr, opts(opt))
    assert ref.hd.get_option("last_adjoint") == L.ADJ_CHAIN_WG
    lerr = abs(float(info["loss_rows"][r]) - float(lr)) / float(lr)
    print(sid, opt, r, counts(info, r), cr, "grad", (info["dp_rows"][r] - gr).abs().max().item(), "loss", lerr,
          "bar", 4 * 35 * N * U24)
    assert counts(info, r) == cr
    assert torch.equal(info["dp_rows"][r], gr)
    assert torch.equal(info["du0"][r:r + 1], du0r.reshape(1, N))
    assert torch.equal(info["u_save"][:, r:r + 1], ur)
    assert lerr <= 4 * 35 * N * U24


CASES = [(s, o) for s in ("S1", "S4", "S5", "S6", "LV") for o in ("fixed", "default")]


@pytest.mark.parametrize("sid,opt", CASES, ids=[f"{s}-{o}" for s, o in CASES])
def test_every_row_is_bitwise_the_two_launch_batch_1_gradient(sid, opt):
    """dp_rows[r], du0[r] and the u_save columns torch.equal, the six step counts ==, for every r.  The two-launch
    path forms its MSE in torch in float (the kernel sums the squares in double and rounds once), so loss_rows[r] is
    held to 4·n·2⁻²⁴ relative with n = 35·N: the fp64 file's bar at float's unit roundoff."""
    rhs, p, u0, X, loss, dp, info = call(sid, opt)
    assert info["stop"] == ["ok"] * 9 and info["dp_rows"].shape == (9, rhs.hd.P)
    assert torch.isfinite(info["dp_rows"]).all() and torch.isfinite(info["u_save"]).all()
    for r in range(9):
        check_row_against_two_launch(sid, opt, rhs, p, u0, X, info, r)
    # (two_launch is native_mse_gradient with du0 kept)
    l0, g0, _ = native_mse_gradient(ref_rhs(sid), u0[0:1].contiguous(), SPAN, p, TS, opts(opt),
                                    X[:, 0:1].contiguous())
    assert torch.equal(g0, info["dp_rows"][0])
    assert not torch.equal(info["dp_rows"][0], info["dp_rows"][1])


@pytest.mark.parametrize("R", [1, 9, 64, 65, 1030])
def test_the_reduction_order(R):
    """dp and loss bitwise the float32 numpy restatement of the chunk-of-64 order on the returned rows (1030: 17
    chunks, the last of 6), and bitwise combine_trajectory_rows on them: the host path's total of the same rows."""
    rhs, p, u0, X, loss, dp, info = call("S1", "default", R=R)
    assert info["stop"] == ["ok"] * R
    rows = rows_of(info)
    assert rows.dtype == np.float32
    want = chunk_order_mean_f32(rows)
    got = np.concatenate([dp.cpu().numpy(), np.array([loss], dtype=np.float64).astype(np.float32)])
    assert float(got[-1]) == loss   # (the double the entry returns is the float total, widened)
    print(R, "vs restated", np.abs(got - want).max(), "vs float64 mean", np.abs(got - rows.astype(np.float64).mean(0)).max())
    assert np.array_equal(got, want)
    host = combine_trajectory_rows(torch.as_tensor(rows)).numpy()
    assert np.array_equal(got, host)
    # the total against mse_loss over the whole tensor in double: every mse_r is rounded to float once (u), a chunk
    # takes at most 64 rounded adds of positive terms, the chunk sums chunks(R) more, the division one: (66 + chunks)·u
    # to first order (1 % for the higher orders; the double sums inside a trajectory are far below u)
    whole = float(kanode.mse_loss(info["u_save"].double(), X.double()))
    print(R, "vs whole-tensor mse", abs(loss - whole) / whole, "bar", (66 + (R + 63) // 64) * U24 * 1.01)
    assert abs(loss - whole) <= (66 + (R + 63) // 64) * U24 * 1.01 * whole


def test_two_launch_groups():
    """S1 at the default tolerances: the capacity is what fits, 1024 steps, a trajectory's float block is 58 KB and
    the 256 MiB buffer holds a group of G (a multiple of 64) trajectories.  R = G + 64 runs as two launches: rows
    0, G - 1, G and R - 1 are bitwise the two-launch path's, and dp is the restated reduction of all rows.  (The
    group is left at its real size: a smaller fused_solve_cap would only make the group larger.)"""
    rhs, p, _ = problem("S1", F32)
    o = opts("default")
    G = rhs.hd.trajectories_gradient_f32_group(0.0, 3.5, 35, o.to_c())
    print("group", G)
    assert 64 <= G <= 65536 - 64 and G % 64 == 0
    R = G + 64
    u0 = t(np.random.default_rng(21).uniform(0.5, 2.0, (R, 2)), F32)
    X = target(R, 2)
    loss, dp, info = rhs.hd.trajectories_gradient_f32_tsit5(p, u0, 0.0, 3.5, TS, X, o.to_c(), rows=True, du0=True,
                                                            u_save=True)
    assert info["stop"] == ["ok"] * R
    for r in (0, G - 1, G, R - 1):
        check_row_against_two_launch("S1", "default", rhs, p, u0, X, info, r)
    got = np.concatenate([dp.cpu().numpy(), np.array([loss]).astype(np.float32)])
    assert np.array_equal(got, chunk_order_mean_f32(rows_of(info)))
    assert rhs.hd.trajectories_gradient_f32_group(0.0, 3.5, 35, opts("fixed").to_c()) > G   # (350 steps: smaller blocks)


def test_not_the_batched_problem():
    """S1, default tolerances: the nine trajectories take their own step-control decisions: at least two distinct
    forward naccept values, and both trajectories with and without a rejected forward step."""
    rhs, p, u0, X, loss, dp, info = call("S1", "default")
    nacc = [s["naccept"] for s in info["fwd_stats"]]
    nrej = [s["nreject"] for s in info["fwd_stats"]]
    print("forward naccept", nacc, "nreject", nrej)
    assert len(set(nacc)) >= 2
    assert any(x == 0 for x in nrej) and any(x > 0 for x in nrej)


def scaled_problem():
    """test_gpu_traj_grad.py's maxiters construction in float32: rows 1 and 6 scaled by 8 leave the net's active range
    and take few, large steps; the others take the nine-trajectory problem's counts."""
    rhs, p, u0 = problem("S1", F32)
    u0 = u0.clone()
    u0[[1, 6]] *= 8.0
    return rhs, p, u0, target(9, 2)


def grad(rhs, p, u0, X, o):
    return rhs.hd.trajectories_gradient_f32_tsit5(p, u0, 0.0, 3.5, TS, X, o.to_c(), rows=True, du0=True, u_save=True)


def check_stopped(info, loss, dp, free, expect):
    for r in range(9):
        assert info["stop"][r] == expect[r], r
        if expect[r] == "ok":
            for k in ("dp_rows", "loss_rows", "du0"):
                assert torch.equal(info[k][r], free[k][r]), (k, r)
            assert torch.equal(info["u_save"][:, r], free["u_save"][:, r])
            assert counts(info, r) == counts(free, r)
        else:
            assert torch.isnan(info["dp_rows"][r]).all() and torch.isnan(info["loss_rows"][r])
            assert torch.isnan(info["du0"][r]).all()
    assert np.isnan(loss) and torch.isnan(dp).all()


MAXITERS_SOME = 45   # (the fp64 file's value; the printed iteration counts below show who finishes under it)


def test_stops_are_per_trajectory():
    """Status paths, not faults, on the scaled S1 problem at the default tolerances.  maxiters bounds the forward's and
    the adjoint's iterations (accepted + rejected steps), and an adjoint takes at least one step per saveat interval
    (35 here), so at maxiters = 12 every row stops, in the forward solve where that alone takes more than 12
    iterations, else in the adjoint.  At MAXITERS_SOME and at a dense capacity of 4 steps some rows finish and some
    stop: who does follows from the unlimited call's own counts, the finished rows keep that call's bits (which
    test 1's construction ties to the two-launch path), the stopped ones are NaN and so are the totals."""
    rhs, p, u0, X = scaled_problem()
    l_free, dp_free, free = grad(rhs, p, u0, X, opts("default"))
    assert free["stop"] == ["ok"] * 9 and np.isfinite(l_free)
    its = [(counts(free, r)[0] + counts(free, r)[1], counts(free, r)[3] + counts(free, r)[4]) for r in range(9)]
    nacc = [counts(free, r)[0] for r in range(9)]
    print("forward / adjoint iterations", its, "forward naccept", nacc)
    for r in (1, 6):
        check_row_against_two_launch("S1", "default", rhs, p, u0, X, free, r)

    def by_maxiters(m):
        return ["forward_maxiters" if f > m else "adjoint_maxiters" if a > m else "ok" for f, a in its]

    loss, dp, info = grad(rhs, p, u0, X, opts("default", maxiters=12))
    print("maxiters 12", info["stop"])
    assert "ok" not in by_maxiters(12) and len(set(by_maxiters(12))) == 2
    check_stopped(info, loss, dp, free, by_maxiters(12))
    first = by_maxiters(12)[0]
    assert ("trajectory 0: " + ("forward" if first == "forward_maxiters" else "adjoint") + " Tsit5: maxiters") in \
        L.lib().kanode_last_error(rhs.hd._h).decode()
    loss, dp, info = grad(rhs, p, u0, X, opts("default", maxiters=MAXITERS_SOME))
    print("maxiters", MAXITERS_SOME, info["stop"])
    want = by_maxiters(MAXITERS_SOME)
    assert "ok" in want and set(want) != {"ok"}
    check_stopped(info, loss, dp, free, want)
    with rhs.hd.options(fused_solve_cap=4):
        loss, dp, info = grad(rhs, p, u0, X, opts("default"))
    print("capacity 4", info["stop"])
    want = ["ok" if n <= 4 else "dense_capacity" for n in nacc]
    assert "ok" in want and "dense_capacity" in want
    check_stopped(info, loss, dp, free, want)
    # and the next call with the defaults repeats the unlimited call's bits
    l2, dp2, again = grad(rhs, p, u0, X, opts("default"))
    assert l2 == l_free and torch.equal(dp2, dp_free) and torch.equal(again["dp_rows"], free["dp_rows"])


def test_python_surface():
    """trajectories_mse_gradient(f32="device") takes the new entry: path "device", gradient rows and their total
    bitwise those of f32="host" on a chain_wide = 0 handle (a loop of two-launch gradients combined in the same order).
    The per-trajectory losses differ by construction (the kernel sums the squares in double and rounds once, the host
    path is torch's float mse_loss), so they and their total are held to test 1's bar, 4·n·2⁻²⁴ relative.  The default
    call on an fp32 handle still takes the host path."""
    rhs, p, u0, X, loss, dp, info = call("S1", "default")
    o = opts("default")
    ld, gd, idv = kanode.trajectories_mse_gradient(rhs, u0, SPAN, p, TS, X, o, rows=True, f32="device")
    assert idv["path"] == "device" and idv["stop"] == ["ok"] * 9
    assert ld == loss and torch.equal(gd, dp) and torch.equal(idv["dp_rows"], info["dp_rows"])
    lh, gh, ih = kanode.trajectories_mse_gradient(ref_rhs("S1"), u0, SPAN, p, TS, X, o, rows=True, f32="host")
    assert ih["path"] == "host" and ih["stop"] == ["ok"] * 9
    assert torch.equal(idv["dp_rows"], ih["dp_rows"]) and torch.equal(gd, gh)
    bar = 4 * 35 * 2 * U24
    lerr = ((idv["loss_rows"].double() - ih["loss_rows"].double()).abs() / ih["loss_rows"].double()).max().item()
    print("loss rows", lerr, "total", abs(ld - lh) / lh, "bar", bar)
    assert lerr <= bar and abs(ld - lh) <= bar * lh
    for a_, b_ in zip(idv["fwd_stats"] + idv["adj_stats"], ih["fwd_stats"] + ih["adj_stats"]):
        assert all(a_[k] == b_[k] for k in ("naccept", "nreject", "nf"))
    l0, g0, i0 = kanode.trajectories_mse_gradient(rhs, u0[:2].contiguous(), SPAN, p, TS, X[:, :2].contiguous(), o)
    assert i0["path"] == "host"
    # an uncovered fp32 handle falls back under f32="device"
    wide = kanode.ChainRHS(kanode.Chain(kanode.KDense(2, 20, 5), kanode.KDense(20, 2, 5)), dtype=F32, device=device())
    pw = t(np.random.default_rng(9).uniform(-0.3, 0.3, wide.hd.P), F32)
    lw, gw, iw = kanode.trajectories_mse_gradient(wide, u0[:2].contiguous(), SPAN, pw, TS, X[:, :2].contiguous(), o,
                                                  f32="device")
    assert iw["path"] == "host" and np.isfinite(lw)


def test_trajectory_trainer_f32_device():
    """TrajectoryTrainer(f32="device") on S1: one step() is FusedAdam applied to the device gradient, bitwise; with
    sparse_reg the loss and gradient are _with_l1's formula added to the λ = 0 result.  On the fp32 LV handle, 16
    initial conditions against targets from the trained parameters of tests/golden/lv_trained_p_seed1.npy: ten
    iterations lower the loss."""
    import os
    from conftest import ROOT
    rhs, p, u0, X, loss, dp, info = call("S1", "default")
    tr = kanode.TrajectoryTrainer(rhs, u0, SPAN, TS, X, p, eta=WG.ETA, solver=opts("default"), f32="device")
    lv0 = tr.step()
    assert tr.last_info["path"] == "device" and lv0 == loss
    x = p.clone()
    ad = kanode.FusedAdam(WG.ETA)
    ad.update(x, dp.contiguous())
    assert torch.equal(x, tr.p) and tr.p.dtype == F32
    m, v, bp = ad.state[id(x)]
    _, m_end, v_end, bp_end = WG.state(tr)
    assert torch.equal(m, m_end) and torch.equal(v, v_end) and bp == bp_end
    reg = kanode.TrajectoryTrainer(rhs, u0, SPAN, TS, X, p, eta=WG.ETA, solver=opts("default"), sparse_reg=5e-4,
                                   f32="device")
    l1, g1, i1 = reg.loss_and_grad()
    assert i1["path"] == "device"
    l0 = torch.as_tensor(loss, dtype=F32, device=device())
    assert torch.equal(l1, l0 + kanode.reg_loss(p, 5e-4, 0.0)) and torch.equal(g1, dp + 5e-4 * torch.sign(p))
    host = kanode.TrajectoryTrainer(rhs, u0[:2].contiguous(), SPAN, TS, X[:, :2].contiguous(), p, solver=opts("default"))
    assert host.loss_and_grad()[2]["path"] == "host"
    lvr = lv(F32)
    u16 = t(np.random.default_rng(21).uniform(0.5, 2.0, (16, 2)), F32)
    pt = t(np.load(os.path.join(ROOT, "tests", "golden", "lv_trained_p_seed1.npy")), F32)
    X16 = kanode.solve_trajectories(lvr, u16, SPAN, pt, TS).u
    assert torch.isfinite(X16).all() and X16.dtype == F32
    fit = kanode.TrajectoryTrainer(lvr, u16, SPAN, TS, X16, t(P0, F32), eta=WG.ETA, f32="device")
    out = fit.run(10)
    print("loss", out["loss"][0], "->", out["loss"][-1])
    assert fit.last_info["path"] == "device"
    assert all(np.isfinite(out["loss"])) and out["loss"][-1] < out["loss"][0]


def raw_call(hd, p, u0, X, R, n_save=35):
    """The new C entry with sentinel-filled outputs: (status, outputs)."""
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
    st = L.lib().kanode_trajectories_gradient_f32_tsit5(hd._h, _ptr(p), _ptr(u0), R, 0.0, 3.5, sv, n_save, _ptr(X),
                                                        C.byref(o), C.byref(loss), _ptr(dp), _ptr(rows), _ptr(lrows),
                                                        None, None, fst, ast, stop, _stream(hd.device))
    torch.cuda.synchronize()
    return st, (loss.value, dp, rows, lrows, list(stop))


def untouched(out):
    loss, dp, rows, lrows, stop = out
    return loss == 7.0 and bool((dp == 7).all()) and bool((rows == 7).all()) and bool((lrows == 7).all()) and \
        all(s == 7 for s in stop)


def test_refusals():
    """An fp64 handle, the Fisher-KPP field (fp32), a [2,20,2] fp32 chain and an fp32 chain with an odd parameter count
    (KDense(1, 1, 2): P = 3): the raw new entry returns KANODE_ERR_UNSUPPORTED with the outputs untouched, and the
    group is 0; n_traj = 0 and 65537 are invalid on a covered handle."""
    rhs64, p64, u64 = problem("S1", R=2)
    wide = kanode.ChainRHS(kanode.Chain(kanode.KDense(2, 20, 5), kanode.KDense(20, 2, 5)), dtype=F32, device=device())
    fk = kanode.FisherKPPRHS(kanode.Chain(kanode.KDense(1, 1, 5, normalizer="softsign")), nx=26, dx=1.0 / 25, D=0.01,
                             dtype=F32, device=device())
    odd = kanode.ChainRHS(kanode.Chain(kanode.KDense(1, 1, 2)), dtype=F32, device=device())
    assert odd.hd.P == 3
    rng = np.random.default_rng(9)
    cases = [("fp64", rhs64, p64, u64, torch.float64),
             ("wide", wide, t(rng.uniform(-0.3, 0.3, wide.hd.P), F32), t(rng.uniform(0.5, 2.0, (2, 2)), F32), F32),
             ("fk", fk, t(rng.uniform(-0.3, 0.3, fk.hd.P), F32), t(rng.uniform(0.1, 0.9, (2, 26)), F32), F32),
             ("odd", odd, t(rng.uniform(-0.3, 0.3, 3), F32), t(rng.uniform(0.5, 2.0, (2, 1)), F32), F32)]
    for name, rhs, p, u0, dt in cases:
        hd = rhs.hd
        X = t(np.random.default_rng(5).uniform(0.5, 2, (35, 2, hd.N)), dt)
        assert not hd.trajectories_gradient_f32_supported(), name
        assert hd.trajectories_gradient_f32_group(0.0, 3.5, 35, kanode.Tsit5Options().to_c()) == 0, name
        st, out = raw_call(hd, p, u0, X, 2)
        print(name, st, L.lib().kanode_last_error(hd._h).decode()[:80])
        assert st == L.ERR_UNSUPPORTED and untouched(out), name
        with pytest.raises(L.KanodeError, match="not supported"):
            hd.trajectories_gradient_f32_tsit5(p, u0, 0.0, 3.5, TS, X, kanode.Tsit5Options().to_c())
    # the fp64 handle keeps its own entry
    assert rhs64.hd.trajectories_gradient_supported()
    rhs, p, u0 = problem("S1", F32)
    X = target(9, 2)
    for R in (0, 65537):
        st, out = raw_call(rhs.hd, p, u0, X, R)
        assert st == L.ERR_INVALID_ARG and untouched(out), R


def test_the_handles_other_paths_keep_their_bits():
    """solve_tsit5, native_mse_gradient and solve_trajectories_tsit5 on the same fp32 handle give the same bits before
    and after a call of the new entry, and the entry repeats its own bits after them."""
    rhs = WG.make_rhs("S1", F32)
    _, p, u0 = problem("S1", F32)
    X = target(9, 2)
    o = opts("default")

    def others():
        a = rhs.hd.solve_tsit5(p, u0[0:1].contiguous(), 0.0, 3.5, TS, o.to_c())[:2]
        b = rhs.hd.solve_trajectories_tsit5(p, u0, 0.0, 3.5, TS, o.to_c())
        l, g, sol = native_mse_gradient(rhs, u0[2:3].contiguous(), SPAN, p, TS, o, X[:, 2:3].contiguous())
        return a, b, (l, g, sol.u)

    a0, b0, c0 = others()
    loss, dp, info = rhs.hd.trajectories_gradient_f32_tsit5(p, u0, 0.0, 3.5, TS, X, o.to_c(), rows=True)
    assert info["stop"] == ["ok"] * 9
    a1, b1, c1 = others()
    assert torch.equal(a0[0], a1[0]) and a0[1] == a1[1]
    assert torch.equal(b0[0], b1[0]) and b0[1] == b1[1] and b0[2] == b1[2]
    for x, y in zip(c0, c1):
        assert torch.equal(x, y)
    loss2, dp2, info2 = rhs.hd.trajectories_gradient_f32_tsit5(p, u0, 0.0, 3.5, TS, X, o.to_c(), rows=True)
    assert loss2 == loss and torch.equal(dp2, dp) and torch.equal(info2["dp_rows"], info["dp_rows"])
