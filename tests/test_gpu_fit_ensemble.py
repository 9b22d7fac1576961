"""Ensemble training of every small chain: R device-resident loops of kd_chain_train_wg_kernel in one launch, one
workgroup per replica (kanode_fit_ensemble_tsit5, kd_chain_train_wg_ens_kernel; EnsembleTrainer(device_loop="any")).
A replica runs the single-replica kernel's body on its own arguments, so except where noted every check is bitwise:
replica r against a fresh Trainer(device_loop="any") from the same p0, eta and λ -- a twin that
tests/test_gpu_train_wg.py pins to the two-launch path and to the C port.

The shapes S1-S6, their data and the solver settings are tests/test_gpu_train_wg.py's: the smallest shapes that reach
each path of the kernel."""
import numpy as np
import pytest
import torch

from gpu_util import device, t
from oracle import oracle as O
from test_gpu_train_wg import ALL, OPTS, SHAPES, TS, TS_TEST, data, lv_rhs, make_rhs, run3, specs_of, state, trainer

import kanode
from kanode import _lib as L

pytestmark = pytest.mark.gpu

SCALES = (1.0, 0.9, 1.1)
ETAS = [1e-3, 5e-4, 2e-3]
LAMS = [0.0, 5e-4, 1e-3]
KEYS = ("loss", "grad", "p_before", "counts")


def p0s_of(sid, scales=SCALES):
    return [data(sid)[0] * s for s in scales]


def ens_of(sid, rhs, p0s, etas, lams, opt, **kw):
    _, u0, X = data(sid)
    kw.setdefault("device_loop", "any")
    return kanode.EnsembleTrainer(rhs, t(u0), (0.0, 3.5), TS, t(X), t(np.stack(p0s)), eta=etas, sparse_reg=lams,
                                  solver=kanode.Tsit5Options(**OPTS[opt]), **kw)


def one_of(sid, rhs, p0, eta, lam, opt):
    _, u0, X = data(sid)
    return kanode.Trainer(rhs, t(u0), (0.0, 3.5), TS, t(X), t(p0), eta=eta, sparse_reg=lam,
                          solver=kanode.Tsit5Options(**OPTS[opt]), device_loop="any")


def same_state(ens, r, st, history):
    p, m, v, bp = st
    assert torch.equal(ens.p[r], p) and torch.equal(ens.m[r], m) and torch.equal(ens.v[r], v), r
    assert ens.bp[r] == list(bp) and ens.history[r] == history, r


def same_run(out, r, o, keys=KEYS):
    for key in keys:
        assert torch.equal(out[key][r], o[key]), (r, key)


def check_replica(ens, out, r, tr, o, keys=KEYS):
    assert tr.last_run == "device_adjoint"
    same_run(out, r, o, keys)
    same_state(ens, r, state(tr), tr.history)


def test_test_files_shapes_are_covered():
    """S1-S6 are shapes of the new entry, whatever the option says, and the option is left alone by the question."""
    for sid in ALL:
        rhs = make_rhs(sid)
        assert rhs.hd.fit_ensemble_supported(SHAPES[sid][2]) and rhs.hd.get_option("train_any_chain") == 0, sid
        assert not rhs.hd.train_supported(SHAPES[sid][2])


@pytest.mark.parametrize("sid,opt", [(s, o) for s in ALL for o in ("fixed", "default")])
def test_replica_equals_single_run(sid, opt):
    """R = 3 from p0·(1, 0.9, 1.1) at three learning rates and penalties, run(3, record=True): every record, p, m, v,
    the running powers and the history of replica r equal its single run's.  (Replica 0 is the run
    tests/test_gpu_train_wg.py shares among its own checks.)"""
    out0, st0, rhs = run3(sid, opt)
    p0s = p0s_of(sid)
    ens = ens_of(sid, rhs, p0s, ETAS, LAMS, opt)
    out = ens.run(3, record=True)
    P = rhs.hd.P
    assert ens.last_run == "device_adjoint" and out["iters_done"] == [3, 3, 3] and out["stop"] == ["ok"] * 3
    assert out["loss"].shape == (3, 3) and out["grad"].shape == (3, 3, P) and out["counts"].shape == (3, 3, 4)
    assert rhs.hd.get_l1_penalty() == 0.0
    same_run(out, 0, out0)
    same_state(ens, 0, st0, out0["loss"].tolist())
    for r in (1, 2):
        tr = one_of(sid, rhs, p0s[r], ETAS[r], LAMS[r], opt)
        check_replica(ens, out, r, tr, tr.run(3, record=True))
    for a_, b_ in ((0, 1), (0, 2), (1, 2)):
        assert not torch.equal(out["loss"][a_], out["loss"][b_]) and not torch.equal(ens.p[a_], ens.p[b_])


@pytest.mark.parametrize("sid", ["S1", "S3"])
def test_one_replica_equals_trainer_run(sid):
    out0, st0, rhs = run3(sid, "default")
    ens = ens_of(sid, rhs, p0s_of(sid)[:1], 1e-3, 0.0, "default")
    out = ens.run(3, record=True)
    assert ens.last_run == "device_adjoint" and out["iters_done"] == [3]
    same_run(out, 0, out0)
    same_state(ens, 0, st0, out0["loss"].tolist())


def test_replica_1_iteration_0_matches_the_c_port():
    """Against the oracle, not project code: replica 1 (not 0) of S3 at dt = 0.01, iteration 0, against
    oracle/cpu_epoch.c, at the bars of test_iteration_0_matches_the_c_port_fixed_step: gradient within 1e-9 of its
    max, loss within 1e-12 relative, p_before[1] within 1e-9·eta.  (The C port has no L1 term: λ = 0 here.)"""
    sid, eta = "S3", 5e-4
    _, u0, X = data(sid)
    p0s = p0s_of(sid)
    lc, gc, pn, st, _ = O.chain_epoch(specs_of(sid), p0s[1].copy(), u0, 3.5, TS, X, adaptive=False, dt=0.01, eta=eta)
    ens = ens_of(sid, make_rhs(sid), p0s, [1e-3, eta, 2e-3], 0.0, "fixed")
    out = ens.run(2, record=True)
    gerr = np.abs(out["grad"][1, 0].cpu().numpy() - gc).max() / np.abs(gc).max()
    lerr = abs(out["loss"][1, 0].item() - lc) / lc
    perr = np.abs(out["p_before"][1, 1].cpu().numpy() - pn).max()
    print(out["counts"][1, 0].tolist(), st, "grad", gerr, "loss", lerr, "p", perr)
    assert out["counts"][1, 0].tolist() == [350, 0, 350, 0]
    assert [st["naccept"], st["nreject"], st["adjoint_naccept"], st["adjoint_nreject"]] == [350, 0, 350, 0]
    assert gerr <= 1e-9
    assert lerr <= 1e-12
    assert perr <= 1e-9 * eta


@pytest.mark.parametrize("sid", ["S1", "S5"])
def test_test_problem(sid):
    """With the test problem over (0, 7): loss_test per replica equals the single run's, and the training results
    keep the bits they have without it."""
    rhs = make_rhs(sid)
    B, N = SHAPES[sid][2], SHAPES[sid][0][0]
    test = ((0.0, 7.0), TS_TEST, t(np.random.default_rng(12).uniform(0.5, 2.0, (71, B, N))))
    p0s = p0s_of(sid)
    plain = ens_of(sid, rhs, p0s, ETAS, LAMS, "default")
    op = plain.run(3, record=True)
    assert op["loss_test"] is None
    ens = ens_of(sid, rhs, p0s, ETAS, LAMS, "default")
    out = ens.run(3, test=test, record=True)
    assert ens.last_run == "device_adjoint" and out["loss_test"].shape == (3, 3)
    assert bool(torch.isfinite(out["loss_test"]).all())
    for key in KEYS:
        assert torch.equal(out[key], op[key]), key
    assert torch.equal(ens.p, plain.p)
    for r in range(3):
        tr = one_of(sid, rhs, p0s[r], ETAS[r], LAMS[r], "default")
        check_replica(ens, out, r, tr, tr.run(3, test=test, record=True), KEYS + ("loss_test",))


def test_one_replica_stops_the_others_finish():
    """Replica 1's p0 has an entry that is exactly 0.0: with a penalty its loss is NaN by the documented rule
    (KANODE_TRAIN_LOSS_NOT_FINITE at iteration 0 -- a status path, not a fault).  run does not raise, replica 1 is
    untouched, replicas 0 and 2 are bitwise their single runs, and the next run launches the two live replicas."""
    sid = "S2"
    rhs = make_rhs(sid)
    p0s = p0s_of(sid)
    p0s[1] = p0s[1].copy()
    p0s[1][17] = 0.0
    ens = ens_of(sid, rhs, p0s, ETAS, 5e-4, "default")
    out = ens.run(3)
    assert ens.last_run == "device_adjoint"
    assert ens.stopped == {1: (0, "loss_not_finite")}
    assert out["iters_done"] == [3, 0, 3] and out["stop"] == ["ok", "loss_not_finite", "ok"]
    assert torch.equal(ens.p[1], t(p0s[1])) and not ens.m[1].any() and not ens.v[1].any()
    assert ens.bp[1] == [0.9, 0.999] and ens.history[1] == [] and bool(torch.isnan(out["loss"][1]).all())
    refs = {r: one_of(sid, rhs, p0s[r], ETAS[r], 5e-4, "default") for r in (0, 2)}
    for r, tr in refs.items():
        assert torch.equal(out["loss"][r], tr.run(3)["loss"])
        same_state(ens, r, state(tr), tr.history)
    out2 = ens.run(2, record=True)
    assert out2["iters_done"] == [2, 0, 2] and ens.live() == [0, 2] and ens.best()[0] in (0, 2)
    assert torch.equal(ens.p[1], t(p0s[1])) and bool(torch.isnan(out2["loss"][1]).all())
    for r, tr in refs.items():
        check_replica(ens, out2, r, tr, tr.run(2, record=True))


def test_state_carries_across_launches():
    """run(2) then run(3, chunk=2) (launches of 2, 2, 1 iterations) equals the Trainers' run(5), bit for bit."""
    sid = "S2"
    rhs = make_rhs(sid)
    p0s = p0s_of(sid)
    ens = ens_of(sid, rhs, p0s, ETAS, LAMS, "default")
    a = ens.run(2, record=True)
    b = ens.run(3, chunk=2, record=True)
    assert a["iters_done"] == [2] * 3 and b["iters_done"] == [3] * 3
    for r in range(3):
        tr = one_of(sid, rhs, p0s[r], ETAS[r], LAMS[r], "default")
        o = tr.run(5, record=True)
        for key in KEYS:
            assert torch.equal(torch.cat([a[key][r], b[key][r]]), o[key]), (r, key)
        same_state(ens, r, state(tr), tr.history)


@pytest.mark.parametrize("sid,opt,cap", [("S1", "default", 128), ("S3", "fixed", 1024)])
def test_where_the_data_lives(sid, opt, cap):
    """KANODE_OPT_FUSED_SOLVE_CAP moves data between LDS and each replica's private global block and changes the
    block's size.  S1 at the default tolerances: by default 1024 steps, whose dense output the WideModel adjoint reads
    from global memory; at 128 steps it is staged in LDS (stage_rec flips).  S3 at dt = 0.01: by default blocks of
    exactly 350 steps, at 1024 steps blocks three times as far apart.  The results are bitwise those of the default
    capacity, and a replica that read a neighbour's block would differ from its single run."""
    rhs = make_rhs(sid)
    p0s = p0s_of(sid)
    a = ens_of(sid, rhs, p0s, ETAS, LAMS, opt)
    oa = a.run(2, record=True)
    b = ens_of(sid, rhs, p0s, ETAS, LAMS, opt)
    with rhs.hd.options(fused_solve_cap=cap):
        ob = b.run(2, record=True)
    assert oa["iters_done"] == ob["iters_done"] == [2, 2, 2] and b.last_run == "device_adjoint"
    for key in KEYS:
        assert torch.equal(oa[key], ob[key]), key
    assert torch.equal(a.p, b.p) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
    for r in (1, 2):
        tr = one_of(sid, rhs, p0s[r], ETAS[r], LAMS[r], opt)
        check_replica(b, ob, r, tr, tr.run(2, record=True))


def test_cotangent_in_each_replicas_global_block():
    """At the 35-row saveat list u_save / dl of S3 always fits in LDS (the capacity ends at 1024 steps), so dl_lds
    flips only with a longer list: 420 rows of 32 entries are 105 KB, which leaves LDS for every replica's own global
    block, behind its dense output.  R = 3 at dt = 0.05, two iterations, against the single runs."""
    sid = "S3"
    rhs = make_rhs(sid)
    _, u0, _ = data(sid)
    ts = [3.5 * i / 419 for i in range(420)]
    X = t(np.random.default_rng(13).uniform(0.5, 2.0, (420, 16, 2)))
    solver = kanode.Tsit5Options(adaptive=False, dt=0.05)
    p0s = p0s_of(sid)
    ens = kanode.EnsembleTrainer(rhs, t(u0), (0.0, 3.5), ts, X, t(np.stack(p0s)), eta=ETAS, sparse_reg=LAMS,
                                 solver=solver, device_loop="any")
    out = ens.run(2, record=True)
    assert ens.last_run == "device_adjoint" and out["iters_done"] == [2, 2, 2]
    for r in range(3):
        tr = kanode.Trainer(rhs, t(u0), (0.0, 3.5), ts, X, t(p0s[r]), eta=ETAS[r], sparse_reg=LAMS[r], solver=solver,
                            device_loop="any")
        check_replica(ens, out, r, tr, tr.run(2, record=True))
    assert not torch.equal(out["loss"][0], out["loss"][1])


def test_more_replicas_than_compute_units():
    sid = "S1"
    cus = torch.cuda.get_device_properties(device()).multi_processor_count
    R = cus + 4
    p0 = data(sid)[0]
    p0s = p0[None, :] + 0.01 * np.random.default_rng(21).normal(size=(R, p0.size))
    rhs = make_rhs(sid)
    ens = ens_of(sid, rhs, list(p0s), 1e-3, 0.0, "fixed")
    out = ens.run(1, record=True)
    assert ens.last_run == "device_adjoint" and out["iters_done"] == [1] * R and ens.stopped == {}
    for r in (0, cus - 1, cus, R - 1):
        tr = one_of(sid, rhs, p0s[r], 1e-3, 0.0, "fixed")
        check_replica(ens, out, r, tr, tr.run(1, record=True))


def test_two_launch_groups():
    """S3 at a capacity of 1024 steps: about 1.8 MB of private block a replica, so the 256 MiB cap splits R = G + 8
    replicas into two launches; the caller sees one call and dense outputs."""
    sid = "S3"
    rhs = make_rhs(sid)
    solver = kanode.Tsit5Options(adaptive=False, dt=0.05)
    _, u0, X = data(sid)
    p0 = data(sid)[0]
    with rhs.hd.options(fused_solve_cap=1024):
        G = rhs.hd.fit_ensemble_group(16, 0.0, 3.5, len(TS), 0, solver.to_c())
        assert 8 < G < 1024, G
        R = G + 8
        p0s = p0[None, :] + 0.01 * np.random.default_rng(22).normal(size=(R, p0.size))
        ens = kanode.EnsembleTrainer(rhs, t(u0), (0.0, 3.5), TS, t(X), t(p0s), eta=1e-3, solver=solver,
                                     device_loop="any")
        out = ens.run(1, record=True)
        assert ens.last_run == "device_adjoint" and out["iters_done"] == [1] * R and ens.stopped == {}
        assert out["counts"][:, 0].tolist() == [[70, 0, 70, 0]] * R
        for r in (G - 1, G, R - 1):
            tr = kanode.Trainer(rhs, t(u0), (0.0, 3.5), TS, t(X), t(p0s[r]), eta=1e-3, solver=solver,
                                device_loop="any")
            check_replica(ens, out, r, tr, tr.run(1, record=True))
    # the group size follows the problem: no fit, no group
    assert rhs.hd.fit_ensemble_group(17, 0.0, 3.5, len(TS), 0, solver.to_c()) == 0
    assert lv_rhs().hd.fit_ensemble_group(1, 0.0, 3.5, len(TS), 0, solver.to_c()) == 0


def test_sandwich_on_one_handle():
    """Trainer.run -> an ensemble run -> Trainer.run on ONE handle equals the uninterrupted Trainer on a handle of
    its own: the handle's buffer regrows for the ensemble and its cached saveat lists and jump groups move, and the
    single run after it must find its own again."""
    sid = "S3"
    rhs, ref_rhs = make_rhs(sid), make_rhs(sid)
    p0s = p0s_of(sid)
    tr = trainer(sid, rhs, device_loop="any")
    a = tr.run(2, record=True)
    ens = ens_of(sid, rhs, p0s, ETAS, LAMS, "default")
    eo = ens.run(2, record=True)
    b = tr.run(2, record=True)
    assert tr.last_run == "device_adjoint" == ens.last_run
    ref = trainer(sid, ref_rhs, device_loop="any")
    ra, rb = ref.run(2, record=True), ref.run(2, record=True)
    for key in KEYS:
        assert torch.equal(a[key], ra[key]) and torch.equal(b[key], rb[key]), key
    for x, y in zip(state(tr)[:3], state(ref)[:3]):
        assert torch.equal(x, y)
    assert state(tr)[3] == state(ref)[3] and tr.history == ref.history
    # and the ensemble in the middle is what it is on a fresh handle
    tr1 = one_of(sid, ref_rhs, p0s[1], ETAS[1], LAMS[1], "default")
    check_replica(ens, eo, 1, tr1, tr1.run(2, record=True))


def test_coverage():
    """The new entry raises "not supported" on the LV handle at B = 1 (pointing to kanode_train_ensemble_tsit5), on
    fp32, at B = 17 and on [2,20,2], with nothing launched; EnsembleTrainer(device_loop="any") on the LV handle
    equals the default EnsembleTrainer bit for bit; on fp32 it takes the host path and equals R step() loops."""
    oc = kanode.Tsit5Options().to_c()
    rng = np.random.default_rng(8)
    R = 2
    rhs1 = make_rhs("S1")
    rhs32 = make_rhs("S1", torch.float32)
    wide = kanode.ChainRHS(kanode.Chain(kanode.KDense(2, 20, 5), kanode.KDense(20, 2, 5)), device=device())
    for f, B, dt, text in ((lv_rhs(), 1, torch.float64, "kanode_train_ensemble_tsit5"),
                           (rhs32, 1, torch.float32, "not supported"), (rhs1, 17, torch.float64, "not supported"),
                           (wide, 1, torch.float64, "not supported")):
        assert not f.hd.fit_ensemble_supported(B)
        u0 = t(rng.uniform(0.5, 2.0, (B, f.N)), dt)
        tg = t(rng.uniform(0.5, 2.0, (35, B, f.N)), dt)
        p = t(rng.uniform(-0.3, 0.3, (R, f.P)), dt)
        keep = p.clone()
        with pytest.raises(L.KanodeError, match="not supported") as err:
            f.hd.fit_ensemble_tsit5(p, torch.zeros_like(p), torch.zeros_like(p), u0, 0.0, 3.5, TS, tg, oc,
                                    [1e-3] * R, (0.9, 0.999), 1e-8, [(0.9, 0.999)] * R, 2)
        assert text in str(err.value) and torch.equal(p, keep)
    assert rhs1.hd.fit_ensemble_supported(16) and rhs1.hd.get_option("train_any_chain") == 0
    # the LV handle: "any" keeps the Lotka-Volterra entry and its bits
    p = rng.uniform(-0.3, 0.3, (3, 240))
    u0 = rng.uniform(0.5, 2.0, (1, 2))
    X = rng.uniform(0.5, 2.0, (35, 1, 2))
    res = []
    for loop in ("default", "any"):
        ens = kanode.EnsembleTrainer(lv_rhs(), t(u0), (0.0, 3.5), TS, t(X), t(p), eta=ETAS, sparse_reg=LAMS,
                                     device_loop=loop)
        out = ens.run(3, record=True)
        assert ens.last_run == "device_adjoint" and out["iters_done"] == [3, 3, 3]
        res.append([out[key] for key in KEYS] + [ens.p.clone(), ens.m.clone(), ens.v.clone()])
    for a_, b_ in zip(*res):
        assert torch.equal(a_, b_)
    # fp32: the host path, R loops of step()
    u0 = t(rng.uniform(0.5, 2.0, (1, 2)), torch.float32)
    tg = t(rng.uniform(0.5, 2.0, (35, 1, 2)), torch.float32)
    p = t(rng.uniform(-0.3, 0.3, (R, rhs32.P)), torch.float32)
    ens = kanode.EnsembleTrainer(rhs32, u0, (0.0, 3.5), TS, tg, p, eta=ETAS[:R], device_loop="any")
    out = ens.run(2)
    assert ens.last_run == "host" and out["iters_done"] == [2, 2]
    for r in range(R):
        b = kanode.Trainer(rhs32, u0, (0.0, 3.5), TS, tg, p[r], eta=ETAS[r])
        ls = [b.step(), b.step()]
        assert torch.equal(ens.p[r], b.p) and out["loss"][r].tolist() == ls == ens.history[r]
