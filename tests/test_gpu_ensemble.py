"""Ensemble training: R independent device-resident loops in one launch, one workgroup per replica
(kanode_train_ensemble_tsit5, kanode_train_forward_ensemble_tsit5; kanode.EnsembleTrainer).  A replica runs the
single-replica kernel's body on its own arguments, so every check here is bitwise: replica r of an ensemble against a
fresh Trainer(...).run(...) from the same p0, eta and λ.

The Lotka-Volterra problem, P0 and OPTS are tests/test_gpu_train_loop.py's; the Fisher-KPP cases are "a" (26, 1, 10)
and "c" (26, 3, 10: two entries per lane, the accumulators in each replica's own global block) of
tests/test_gpu_fk_train_loop.py."""
import numpy as np
import pytest
import torch

import test_gpu_fk_train_loop as FK
from gpu_util import device, t
from test_gpu_train_loop import OPTS, P0, TS, TS_TEST, U0, X, X_TEST, lv

import kanode
from kanode import _lib as L

pytestmark = pytest.mark.gpu

ETAS = [1e-3, 5e-4, 2e-3]
LAMS = [0.0, 5e-4, 1e-3]
KEYS = ("loss", "grad", "p_before", "counts")


def lv_p0(seed):
    if seed == 4:
        return P0
    return kanode.Chain(kanode.KDense(2, 10, 5), kanode.KDense(10, 2, 5)).setup(np.random.default_rng(seed))[0].astype(
        np.float64) / 10


LV_P0S = [lv_p0(s) for s in (4, 5, 6)]


def lv_ens(rhs, p0s, etas, lams, opt):
    return kanode.EnsembleTrainer(rhs, t(U0), (0.0, 3.5), TS, t(X), t(np.stack(p0s)), eta=etas,
                                  solver=kanode.Tsit5Options(**OPTS[opt]), sparse_reg=lams)


def lv_one(rhs, p0, eta, lam, opt):
    return kanode.Trainer(rhs, t(U0), (0.0, 3.5), TS, t(X), t(p0), eta=eta, solver=kanode.Tsit5Options(**OPTS[opt]),
                          sparse_reg=lam)


def fk_p0s(case, n):
    pr = FK.problem(case)
    rng = np.random.default_rng(90)
    return [pr["p0"] + (0.05 * rng.normal(size=pr["p0"].shape) if r else 0.0) for r in range(n)]


def fk_ens(case, rhs, p0s, etas, opt, lams=0.0):
    pr = FK.problem(case)
    return kanode.EnsembleTrainer(rhs, t(pr["u0"]), FK.TSPAN, FK.SAVEAT, t(pr["X"]), t(np.stack(p0s)), eta=etas,
                                  solver=kanode.Tsit5Options(**FK.OPTS[opt]), sparse_reg=lams)


def fk_one(case, rhs, p0, eta, opt):
    pr = FK.problem(case)
    return kanode.Trainer(rhs, t(pr["u0"]), FK.TSPAN, FK.SAVEAT, t(pr["X"]), t(p0), eta=eta,
                          solver=kanode.Tsit5Options(**FK.OPTS[opt]))


def same_state(ens, r, tr):
    m, v, bp = tr.opt.state[id(tr.p)]
    assert torch.equal(ens.p[r], tr.p) and torch.equal(ens.m[r], m) and torch.equal(ens.v[r], v)
    assert ens.bp[r] == list(bp) and ens.history[r] == tr.history


def same_run(out, r, o, keys=KEYS):
    for key in keys:
        assert torch.equal(out[key][r], o[key]), (r, key)


@pytest.mark.parametrize("opt", ["fixed", "default"])
def test_lv_replica_equals_single_run(opt):
    rhs = lv()
    ens = lv_ens(rhs, LV_P0S, ETAS, LAMS, opt)
    out = ens.run(3, record=True)
    assert ens.last_run == "device_adjoint" and out["iters_done"] == [3, 3, 3] and out["stop"] == ["ok"] * 3
    assert out["loss"].shape == (3, 3) and out["grad"].shape == (3, 3, 240) and out["counts"].shape == (3, 3, 4)
    assert rhs.hd.get_l1_penalty() == 0.0
    for r in range(3):
        tr = lv_one(rhs, LV_P0S[r], ETAS[r], LAMS[r], opt)
        o = tr.run(3, record=True)
        assert tr.last_run == "device_adjoint"
        same_run(out, r, o)
        same_state(ens, r, tr)
    assert not torch.equal(out["loss"][0], out["loss"][1])


@pytest.mark.parametrize("opt", ["fixed", "default"])
@pytest.mark.parametrize("case", ["a", "c"])
def test_fk_replica_equals_single_run(case, opt):
    """Case "c" keeps its accumulators in global memory: a block shared between replicas would show here."""
    rhs = FK.make_rhs(case)
    p0s = fk_p0s(case, 3)
    ens = fk_ens(case, rhs, p0s, ETAS, opt)
    out = ens.run(3, record=True)
    assert ens.last_run == "device_forward" and out["iters_done"] == [3, 3, 3]
    for r in range(3):
        tr = fk_one(case, rhs, p0s[r], ETAS[r], opt)
        o = tr.run(3, record=True)
        assert tr.last_run == "device_forward"
        same_run(out, r, o)
        same_state(ens, r, tr)
    assert not torch.equal(out["loss"][0], out["loss"][1])


@pytest.mark.parametrize("opt", ["fixed", "default"])
def test_one_replica_equals_trainer_run(opt):
    rhs = lv()
    ens = lv_ens(rhs, LV_P0S[:1], 1e-3, 0.0, opt)
    out = ens.run(3, record=True)
    tr = lv_one(rhs, LV_P0S[0], 1e-3, 0.0, opt)
    same_run(out, 0, tr.run(3, record=True))
    same_state(ens, 0, tr)
    frhs = FK.make_rhs("a")
    fe = fk_ens("a", frhs, fk_p0s("a", 1), FK.ETA, opt)
    fout = fe.run(3, record=True)
    ftr = fk_one("a", frhs, fk_p0s("a", 1)[0], FK.ETA, opt)
    same_run(fout, 0, ftr.run(3, record=True))
    same_state(fe, 0, ftr)
    assert fe.last_run == "device_forward" and ens.last_run == "device_adjoint"


def test_dense_output_in_each_replicas_global_block():
    """The 1e-9 tolerance with KANODE_OPT_FUSED_SOLVE_CAP past what LDS holds (every replica's dense output in its
    own global block) against the default capacity (staged in LDS): all results bitwise equal."""
    rhs = lv()
    a = lv_ens(rhs, LV_P0S, ETAS, LAMS, "tight")
    oa = a.run(3, record=True)
    b = lv_ens(rhs, LV_P0S, ETAS, LAMS, "tight")
    with rhs.hd.options(fused_solve_cap=4096):
        ob = b.run(3, record=True)
    assert oa["iters_done"] == ob["iters_done"] == [3, 3, 3]
    for key in KEYS:
        assert torch.equal(oa[key], ob[key]), key
    assert torch.equal(a.p, b.p) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
    tr = lv_one(rhs, LV_P0S[2], ETAS[2], LAMS[2], "tight")
    same_run(ob, 2, tr.run(3, record=True))


@pytest.mark.parametrize("opt", ["fixed", "default"])
def test_test_problem(opt):
    """R = 2 with the (0, 14) test problem: loss_test per replica equals the single run's, and the training results
    keep the bits they have without it."""
    rhs = lv()
    test = ((0.0, 14.0), TS_TEST, t(X_TEST))
    plain = lv_ens(rhs, LV_P0S[:2], ETAS[:2], LAMS[:2], opt)
    op = plain.run(3, record=True)
    assert op["loss_test"] is None
    ens = lv_ens(rhs, LV_P0S[:2], ETAS[:2], LAMS[:2], opt)
    out = ens.run(3, test=test, record=True)
    assert out["loss_test"].shape == (2, 3)
    for key in KEYS:
        assert torch.equal(out[key], op[key]), key
    assert torch.equal(ens.p, plain.p)
    for r in range(2):
        tr = lv_one(rhs, LV_P0S[r], ETAS[r], LAMS[r], opt)
        o = tr.run(3, test=test, record=True)
        same_run(out, r, o, KEYS + ("loss_test",))
        same_state(ens, r, tr)
    # the Fisher-KPP loop's logged-loss solve (its counts fill columns 2 and 3)
    frhs = FK.make_rhs("a")
    pr = FK.problem("a")
    ftest = (FK.TSPAN, FK.SAVEAT, t(pr["X"]))
    p0s = fk_p0s("a", 2)
    fe = fk_ens("a", frhs, p0s, ETAS[:2], opt)
    fout = fe.run(3, test=ftest, record=True)
    for r in range(2):
        tr = fk_one("a", frhs, p0s[r], ETAS[r], opt)
        same_run(fout, r, tr.run(3, test=ftest, record=True), KEYS + ("loss_test",))
        same_state(fe, r, tr)


@pytest.mark.parametrize("opt", ["fixed", "default"])
def test_one_replica_stops_the_others_finish(opt):
    """Replica 1's p0 has an entry that is exactly 0.0: with a penalty its loss is NaN by the documented rule
    (KANODE_TRAIN_LOSS_NOT_FINITE at iteration 0 -- a status path, not a fault).  run does not raise, replica 1 is
    untouched, replicas 0 and 2 are bitwise their single runs, and the next run launches the two live replicas."""
    rhs = lv()
    p0s = [LV_P0S[0], LV_P0S[1].copy(), LV_P0S[2]]
    p0s[1][17] = 0.0
    ens = lv_ens(rhs, p0s, ETAS, 5e-4, opt)
    out = ens.run(3)
    assert ens.stopped == {1: (0, "loss_not_finite")}
    assert out["iters_done"] == [3, 0, 3] and out["stop"] == ["ok", "loss_not_finite", "ok"]
    assert torch.equal(ens.p[1], t(p0s[1])) and not ens.m[1].any() and not ens.v[1].any()
    assert ens.bp[1] == [0.9, 0.999] and ens.history[1] == [] and bool(torch.isnan(out["loss"][1]).all())
    refs = {r: lv_one(rhs, p0s[r], ETAS[r], 5e-4, opt) for r in (0, 2)}
    for r, tr in refs.items():
        assert torch.equal(out["loss"][r], tr.run(3)["loss"])
        same_state(ens, r, tr)
    out2 = ens.run(2, record=True)
    assert out2["iters_done"] == [2, 0, 2] and ens.live() == [0, 2] and ens.best()[0] in (0, 2)
    assert torch.equal(ens.p[1], t(p0s[1])) and bool(torch.isnan(out2["loss"][1]).all())
    for r, tr in refs.items():
        same_run(out2, r, tr.run(2, record=True))
        same_state(ens, r, tr)


def test_more_replicas_than_compute_units():
    cus = torch.cuda.get_device_properties(device()).multi_processor_count
    R = cus + 3
    p0 = P0[None, :] + 0.01 * np.random.default_rng(21).normal(size=(R, P0.size))
    rhs = lv()
    ens = lv_ens(rhs, list(p0), 1e-3, 0.0, "fixed")
    out = ens.run(1, record=True)
    assert out["iters_done"] == [1] * R and ens.stopped == {}
    for r in (0, cus, R - 1):
        tr = lv_one(rhs, p0[r], 1e-3, 0.0, "fixed")
        same_run(out, r, tr.run(1, record=True))
        same_state(ens, r, tr)


@pytest.mark.parametrize("opt", ["fixed", "default"])
def test_state_carries_across_launches(opt):
    """run(3) = run(2); run(1) = run(3, chunk=1), bit for bit, with R = 2."""
    rhs = lv()
    res = []
    for how in ("one", "split", "chunk"):
        ens = lv_ens(rhs, LV_P0S[:2], ETAS[:2], LAMS[:2], opt)
        if how == "one":
            loss = ens.run(3)["loss"]
        elif how == "split":
            loss = torch.cat([ens.run(2)["loss"], ens.run(1)["loss"]], dim=1)
        else:
            loss = ens.run(3, chunk=1)["loss"]
        assert [len(h) for h in ens.history] == [3, 3]
        res.append((ens.p.clone(), ens.m.clone(), ens.v.clone(), loss, ens.bp))
    for other in res[1:]:
        for a_, b_ in zip(res[0][:4], other[:4]):
            assert torch.equal(a_, b_)
        assert res[0][4] == other[4]


def test_coverage_and_fallback():
    """B = 2 on the LV handle, fp32 and a pruned [2, 7, 2] chain are not covered: the raw call raises "not
    supported", and EnsembleTrainer.run takes the host path and equals R Trainer.step() loops bit for bit.  A
    non-zero l1 on the forward entry raises "not supported" as well."""
    rhs = lv()
    rhs32 = lv(torch.float32)
    rhs7 = kanode.ChainRHS(kanode.Chain(kanode.KDense(2, 7, 5), kanode.KDense(7, 2, 5)), device=device())
    oc = kanode.Tsit5Options().to_c()
    rng = np.random.default_rng(8)
    R = 2
    for f, B, dt in ((rhs, 2, torch.float64), (rhs32, 1, torch.float32), (rhs7, 1, torch.float64)):
        u0 = t(rng.uniform(0.5, 2.0, (B, f.N)), dt)
        tg = t(rng.uniform(0.5, 2.0, (35, B, f.N)), dt)
        p = t(rng.uniform(-0.3, 0.3, (R, f.P)), dt)
        with pytest.raises(L.KanodeError, match="not supported"):
            f.hd.train_ensemble_tsit5(p.clone(), torch.zeros_like(p), torch.zeros_like(p), u0, 0.0, 3.5, TS, tg, oc,
                                      [1e-3] * R, (0.9, 0.999), 1e-8, [(0.9, 0.999)] * R, 2)
        ens = kanode.EnsembleTrainer(f, u0, (0.0, 3.5), TS, tg, p, eta=ETAS[:R])
        out = ens.run(2)
        assert ens.last_run == "host" and out["iters_done"] == [2, 2]
        for r in range(R):
            b = kanode.Trainer(f, u0, (0.0, 3.5), TS, tg, p[r], eta=ETAS[r])
            ls = [b.step(), b.step()]
            assert torch.equal(ens.p[r], b.p) and out["loss"][r].tolist() == ls == ens.history[r]
    frhs = FK.make_rhs("a")
    pr = FK.problem("a")
    p = t(np.stack(fk_p0s("a", 2)))
    args = (p, torch.zeros_like(p), torch.zeros_like(p), t(pr["u0"]), 0.0, 2.0, FK.SAVEAT, t(pr["X"]), oc, [1e-2] * 2,
            (0.9, 0.999), 1e-8, [(0.9, 0.999)] * 2, 1)
    with pytest.raises(L.KanodeError, match="not supported"):
        frhs.hd.train_forward_ensemble_tsit5(*args, l1=[0.0, 5e-4])
    assert torch.equal(p, t(np.stack(fk_p0s("a", 2))))                     # nothing was launched
    r = frhs.hd.train_forward_ensemble_tsit5(*args, l1=[0.0, 0.0])
    assert r["iters_done"] == [1, 1] and r["stop"] == ["ok", "ok"] and r["error"] is None
