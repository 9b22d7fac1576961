"""The ensemble solve: R parameter vectors of one problem in one launch, one workgroup per replica
(kanode_solve_ensemble_tsit5; KanodeHandle.solve_ensemble_tsit5, kanode.solve_ensemble, EnsembleTrainer.predict /
eval_loss).  Replica r runs its single-replica twin's device code at p + r·P, so "equal" here is torch.equal on u and
== on the three counts, against hd.solve_tsit5 / kanode.solve at p[r] on the same handle.

The chain shapes S1-S6, their data and solver settings are tests/test_gpu_train_wg.py's, the Lotka-Volterra handle and
P0 tests/test_gpu_train_loop.py's; the Fisher-KPP problems follow tests/test_gpu_fk_train_loop.py's construction
(cases "a" and "c" are its own)."""
import ctypes as C

import numpy as np
import pytest
import torch

import bench
import test_gpu_fk_train_loop as FK
import test_gpu_train_wg as WG
from gpu_util import device, t
from test_gpu_ensemble import ETAS, LAMS, LV_P0S, lv_ens
from test_gpu_train_loop import P0, U0, lv

import kanode
from kanode import _lib as L
from kanode.handle import _ptr, _stream

pytestmark = pytest.mark.gpu

TS, TS_TEST, OPTS = WG.TS, WG.TS_TEST, WG.OPTS
SCALES = [1.0, 0.5, 2.0]
# case: nx, B, G, normalizer ("e": 320 threads, the 1024-bound kernel; "f": a full wave)
FK_CASES = {"a": (26, 1, 10, "softsign"), "c": (26, 3, 10, "softsign"), "e": (8, 5, 5, "tanh_fast"),
            "f": (64, 1, 10, "softsign")}
_RHS = {}


def opts(name, **kw):
    return kanode.Tsit5Options(**dict(OPTS[name], **kw))


def chain_rhs(sid, dtype=torch.float64):
    if (sid, dtype) not in _RHS:
        _RHS[(sid, dtype)] = lv(dtype) if sid == "LV" else WG.make_rhs(sid, dtype)
    return _RHS[(sid, dtype)]


def chain_problem(sid, dtype=torch.float64, scales=SCALES):
    p, u0 = (P0, U0) if sid == "LV" else WG.data(sid)[:2]
    return chain_rhs(sid, dtype), t(np.stack([s * p for s in scales]), dtype), t(u0, dtype)


def fk_problem(case):
    """tests/test_gpu_fk_train_loop.py's problem() for the cases above."""
    nx, B, G, _ = FK_CASES[case]
    rng = np.random.default_rng(11 + ord(case))
    x = np.arange(nx) / nx
    c = rng.uniform(0.3, 0.7, (B, 1))
    d = np.abs(x[None, :] - c)
    u0 = np.exp(-(np.minimum(d, 1.0 - d) / 0.15) ** 2)
    rng.uniform(0.0, 1.0, (len(FK.SAVEAT), B, nx))   # (its target, drawn to keep the stream)
    p0 = bench.fk_trained_like_params() if G == 10 else rng.normal(0.0, 0.3, G + 1)
    r90 = np.random.default_rng(90)
    ps = np.stack([p0 + (0.05 * r90.normal(size=p0.shape) if r else 0.0) for r in range(3)])
    return t(ps), t(u0)


def fk_rhs(case=None, nx=None, G=10, norm="softsign", dtype=torch.float64):
    if case is not None:
        nx, _, G, norm = FK_CASES[case]
    key = ("fk", nx, G, norm, dtype)
    if key not in _RHS:
        kan1 = kanode.Chain(kanode.KDense(1, 1, G, normalizer=norm, basis_func="rbf"))
        _RHS[key] = kanode.FisherKPPRHS(kan1, nx=nx, dx=1.0 / nx, D=0.01, dtype=dtype, device=device())
    return _RHS[key]


def same_as_single(hd, ps, u0, tspan, saveat, o, what=""):
    """One ensemble call; every replica equal to its own solve_tsit5 on the same handle."""
    u, stats, stop = hd.solve_ensemble_tsit5(ps, u0, tspan[0], tspan[1], saveat, o.to_c())
    R = ps.shape[0]
    assert u.shape == (R, len(saveat)) + tuple(u0.shape) and stop == ["ok"] * R
    for r in range(R):
        one, st, _ = hd.solve_tsit5(ps[r].contiguous(), u0, tspan[0], tspan[1], saveat, o.to_c())
        print(what, r, stats[r], st, "bitwise" if torch.equal(u[r], one) else (u[r] - one).abs().max().item())
        assert stats[r] == st
        assert torch.equal(u[r], one)
        assert torch.isfinite(one).all()
    return u, stats


CHAIN_CASES = ([(s, o, torch.float64) for s in WG.ALL + ["LV"] for o in ("fixed", "default")] +
               [("S1", "tight", torch.float64), ("S3", "tight", torch.float64)] +
               [("S6", o, torch.float32) for o in ("fixed", "default")])


@pytest.mark.parametrize("sid,opt,dtype", CHAIN_CASES, ids=[f"{s}-{o}-{str(d)[-2:]}" for s, o, d in CHAIN_CASES])
def test_chain_replicas_equal_their_single_solves(sid, opt, dtype):
    rhs, ps, u0 = chain_problem(sid, dtype)
    assert rhs.hd.solve_ensemble_supported(u0.shape[0])
    u, _ = same_as_single(rhs.hd, ps, u0, (0.0, 3.5), TS, opts(opt), f"{sid} {opt}")
    assert not torch.equal(u[0], u[1])


def test_chain_over_the_test_span():
    rhs, ps, u0 = chain_problem("S2")
    u, stats = same_as_single(rhs.hd, ps, u0, (0.0, 7.0), TS_TEST, opts("default"), "S2 test span")
    assert u.shape == (3, 71, 3, 2) and not torch.equal(u[0], u[1])


def test_anchor_against_the_python_statement_on_the_cpu():
    """S1, fixed step, replica 1 against kanode.solve on the CPU oracle's RHS: the same 350 steps, values within
    1e-11 (the project's native-against-Python-statement bar)."""
    from oracle.oracle_rhs import OracleChainRHS
    rhs, ps, u0 = chain_problem("S1")
    o = opts("fixed")
    u, stats, stop = rhs.hd.solve_ensemble_tsit5(ps, u0, 0.0, 3.5, TS, o.to_c())
    ref = kanode.solve(OracleChainRHS(WG.specs_of("S1")), u0.cpu(), (0.0, 3.5), ps[1].cpu(), TS, o)
    err = (u[1].cpu() - ref.u).abs().max().item()
    print("anchor", stats[1], ref.stats, err)
    assert stats[1] == ref.stats and stats[1]["naccept"] == 350
    assert err <= 1e-11


@pytest.mark.parametrize("opt", ["fixed", "default"])
@pytest.mark.parametrize("case", list(FK_CASES))
def test_fk_replicas_equal_their_single_solves(case, opt):
    rhs = fk_rhs(case)
    ps, u0 = fk_problem(case)
    assert rhs.hd.solve_ensemble_supported(u0.shape[0])
    u, _ = same_as_single(rhs.hd, ps, u0, FK.TSPAN, FK.SAVEAT, kanode.Tsit5Options(**FK.OPTS[opt]), f"fk {case} {opt}")
    assert not torch.equal(u[0], u[1])


@pytest.mark.parametrize("opt,tspan,saveat", [("fixed", (0.0, 0.2), [0.0, 0.1, 0.2]), ("default", FK.TSPAN, FK.SAVEAT)])
def test_fk_off_the_table_takes_the_direct_formula(opt, tspan, saveat):
    """u0 scaled by 4.5 on the 26-point field lies off the table (L <= 4): the direct formula runs in every replica.
    On the CPU oracle the solves stay finite and take 20 (fixed, over (0, 0.2)) and 17-18 (default, over (0, 2))
    steps."""
    rhs = fk_rhs("a")
    ps, u0 = fk_problem("a")
    u0 = (4.5 * u0).contiguous()
    assert u0.max().item() > 4.0
    _, stats = same_as_single(rhs.hd, ps, u0, tspan, saveat, kanode.Tsit5Options(**FK.OPTS[opt]), f"fk off-table {opt}")
    if opt == "fixed":
        assert all(s["naccept"] == 20 for s in stats)


def test_fk_handle_state_is_untouched():
    """solve(p0) -> ensemble solve -> solve(p0) -> rhs(p0, u0): the first results' bits, and the handle's own table and
    stamps as they were (kanode_table_rejections unchanged)."""
    rhs = fk_rhs("a")
    ps, u0 = fk_problem("a")
    p0 = ps[0].contiguous()
    o = kanode.Tsit5Options()
    f0 = rhs.hd.rhs(p0, u0).clone()
    a = kanode.solve(rhs, u0, FK.TSPAN, p0, FK.SAVEAT, o)
    rej = rhs.hd.table_rejections()
    far = torch.cat([ps, ps + 0.3]).contiguous()   # (the replicas above, and tables far from p0's)
    rhs.hd.solve_ensemble_tsit5(far, u0, FK.TSPAN[0], FK.TSPAN[1], FK.SAVEAT, o.to_c())
    assert rhs.hd.table_rejections() == rej
    b = kanode.solve(rhs, u0, FK.TSPAN, p0, FK.SAVEAT, o)
    assert torch.equal(a.u, b.u) and a.stats == b.stats
    assert torch.equal(rhs.hd.rhs(p0, u0), f0)
    assert rhs.hd.table_rejections() == rej


def test_more_replicas_than_compute_units():
    rhs, _, u0 = chain_problem("LV")
    R = 300
    ps = t(np.stack([P0 * (1.0 + 1e-3 * (r % 5)) for r in range(R)]))
    o = opts("fixed")
    sv = [0.0, 0.02, 0.04]
    u, stats, stop = rhs.hd.solve_ensemble_tsit5(ps, u0, 0.0, 0.04, sv, o.to_c())
    assert stop == ["ok"] * R and all(s == stats[0] for s in stats) and stats[0]["naccept"] == 4
    for r in (5, 255, 260, 295):
        assert torch.equal(u[r], u[0])
    assert not torch.equal(u[1], u[0])
    for r in (0, 1, 256, 299):
        one, st, _ = rhs.hd.solve_tsit5(ps[r].contiguous(), u0, 0.0, 0.04, sv, o.to_c())
        assert torch.equal(u[r], one) and stats[r] == st


def test_maxiters_stops_one_replica_on_the_device():
    """tests/test_ensemble_solve_cpu.py's case ([p, 3p, p], default tolerances, maxiters = 12: 6 against 26
    iterations) through the raw entry."""
    rhs, ps, u0 = chain_problem("S1", scales=[1.0, 3.0, 1.0])
    o = opts("default", maxiters=12)
    u, stats, stop = rhs.hd.solve_ensemble_tsit5(ps, u0, 0.0, 3.5, TS, o.to_c())
    print(stats, stop)
    assert stop == ["ok", "maxiters", "ok"]
    assert "replica 1" in L.lib().kanode_last_error(rhs.hd._h).decode()
    assert stats[1]["naccept"] + stats[1]["nreject"] == 12
    assert torch.isnan(u[1]).any()   # (the rows past its last reached stop are as the NaN pre-fill left them)
    one, st, _ = rhs.hd.solve_tsit5(ps[0].contiguous(), u0, 0.0, 3.5, TS, o.to_c())
    for r in (0, 2):
        assert torch.equal(u[r], one) and stats[r] == st
    with pytest.raises(L.KanodeError, match="maxiters"):
        kanode.solve(rhs, u0, (0.0, 3.5), ps[1], TS, o)
    sol = kanode.solve_ensemble(rhs, u0, (0.0, 3.5), ps, TS, o)
    assert sol.path == "device" and sol.stop == stop and torch.isnan(sol.u[1]).all() and torch.equal(sol.u[0], one)


def raw(hd, ps, u0, B, tspan, saveat, n_save=None, R=None, u_save=None, p_null=False):
    """The C entry itself: (status, u_save)."""
    R = ps.shape[0] if R is None else R
    n_save = len(saveat) if n_save is None else n_save
    if u_save is None:
        u_save = torch.full((max(ps.shape[0], 1), max(len(saveat), 1)) + tuple(u0.shape), -7.0, dtype=u0.dtype,
                            device=u0.device)
    sv = (C.c_double * max(1, len(saveat)))(*saveat)
    st = (L.SolveStatsC * max(ps.shape[0], 1))()
    stop = (C.c_int32 * max(ps.shape[0], 1))()
    o = kanode.Tsit5Options().to_c()
    rc = L.lib().kanode_solve_ensemble_tsit5(hd._h, R, None if p_null else _ptr(ps), _ptr(u0), B, tspan[0], tspan[1],
                                             sv, n_save, _ptr(u_save), C.byref(o), st, stop, _stream(hd.device))
    torch.cuda.synchronize()
    return rc, u_save


_NOT_COVERED = []


def not_covered():
    """(name, rhs, ps, u0) of the shapes the one-workgroup solve does not take (made once)."""
    if not _NOT_COVERED:
        _NOT_COVERED.extend(_not_covered())
    return _NOT_COVERED


def _not_covered():
    rng = np.random.default_rng(5)
    rhs, ps, _ = chain_problem("LV")
    yield "B=17", rhs, ps, t(rng.uniform(0.5, 2.0, (17, 2)))
    wide = kanode.ChainRHS(kanode.Chain(kanode.KDense(2, 20, 5), kanode.KDense(20, 2, 5)), dtype=torch.float64,
                           device=device())
    yield "[2,20,2]", wide, t(rng.uniform(-0.1, 0.1, (3, wide.hd.P))), t(U0)
    fps, fu0 = fk_problem("a")
    yield "fp32 fk", fk_rhs("a", dtype=torch.float32), fps.float(), fu0.float()
    for nx in (7, 66):
        x = np.arange(nx) / nx
        yield f"nx={nx}", fk_rhs(nx=nx), fps, t(np.exp(-(np.minimum(x, 1.0 - x)[None, :] / 0.15) ** 2))


@pytest.mark.parametrize("which", range(5))
def test_not_covered_is_refused_and_takes_the_host_path(which):
    name, rhs, ps, u0 = not_covered()[which]
    B = u0.shape[0]
    assert not rhs.hd.solve_ensemble_supported(B)
    rc, u_save = raw(rhs.hd, ps, u0, B, (0.0, 0.5), [0.0, 0.25, 0.5])
    assert rc == L.ERR_UNSUPPORTED and "not supported" in L.lib().kanode_last_error(rhs.hd._h).decode(), name
    assert (u_save == -7.0).all()
    with pytest.raises(L.KanodeError, match="not supported"):
        rhs.hd.solve_ensemble_tsit5(ps, u0, 0.0, 0.5, [0.0, 0.25, 0.5], kanode.Tsit5Options().to_c())
    sol = kanode.solve_ensemble(rhs, u0, (0.0, 0.5), ps, [0.0, 0.25, 0.5])
    assert sol.path == "host" and sol.stop == ["ok"] * 3
    for r in range(3):
        one = kanode.solve(rhs, u0, (0.0, 0.5), ps[r], [0.0, 0.25, 0.5])
        assert torch.equal(sol.u[r], one.u) and sol.stats[r] == one.stats


def test_fused_solve_off_is_not_covered():
    rhs, ps, u0 = chain_problem("LV")
    with rhs.hd.options(fused_solve=0):
        assert not rhs.hd.solve_ensemble_supported(1)
        rc, u_save = raw(rhs.hd, ps, u0, 1, (0.0, 0.5), [0.0, 0.25, 0.5])
        assert rc == L.ERR_UNSUPPORTED and (u_save == -7.0).all()
        sol = kanode.solve_ensemble(rhs, u0, (0.0, 0.5), ps, [0.0, 0.25, 0.5])
        assert sol.path == "host"
        for r in range(3):
            assert torch.equal(sol.u[r], kanode.solve(rhs, u0, (0.0, 0.5), ps[r], [0.0, 0.25, 0.5]).u)
    assert rhs.hd.solve_ensemble_supported(1)


def test_bad_arguments():
    rhs, ps, u0 = chain_problem("LV")
    sv = [0.0, 0.25, 0.5]
    for kw in (dict(R=0), dict(R=4097), dict(p_null=True), dict(n_save=0)):
        rc, u_save = raw(rhs.hd, ps, u0, 1, (0.0, 0.5), sv, **kw)
        assert rc == L.ERR_INVALID_ARG and (u_save == -7.0).all(), kw
    rc, u_save = raw(rhs.hd, ps, u0, 1, (0.0, 0.5), [0.5, 0.25, 0.0])
    assert rc == L.ERR_INVALID_ARG and (u_save == -7.0).all()
    rc, u_save = raw(rhs.hd, ps, u0, 1, (0.0, 0.5), sv)
    assert rc == L.OK and torch.isfinite(u_save).all()


def test_ensemble_trainer_predict_and_eval_loss_on_the_device():
    rhs = lv()
    ens = lv_ens(rhs, LV_P0S, ETAS, LAMS, "default")
    ens.run(2)
    before = (ens.p.clone(), ens.m.clone(), ens.v.clone(), [list(b) for b in ens.bp], [list(h) for h in ens.history])
    X_t = t(np.random.default_rng(13).uniform(0.5, 2.0, (71, 1, 2)))
    sol = ens.predict()
    assert ens.last_predict == "device" and sol.t == TS and sol.u.shape == (3, 35, 1, 2)
    sol_t = ens.predict((0.0, 7.0), TS_TEST)
    assert ens.last_predict == "device" and sol_t.u.shape == (3, 71, 1, 2)
    losses, losses_t = ens.eval_loss(), ens.eval_loss(test=((0.0, 7.0), TS_TEST, X_t))
    for r in range(3):
        m = ens.member(r)
        that = m.predict(m.p).u
        that_t = kanode.solve(rhs, m.u0, (0.0, 7.0), m.p, TS_TEST, m.solver).u
        assert torch.equal(sol.u[r], that) and torch.equal(sol_t.u[r], that_t)
        assert losses[r] == float(kanode.mse_loss(that, m.target))
        assert losses_t[r] == float(kanode.mse_loss(that_t, X_t))
    after = (ens.p, ens.m, ens.v, [list(b) for b in ens.bp], [list(h) for h in ens.history])
    assert all(torch.equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3:] == after[3:]
