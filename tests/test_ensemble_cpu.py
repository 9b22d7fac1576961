"""kanode.EnsembleTrainer on the CPU (its host path: R Trainers stepped in turn) with the torch Lotka-Volterra RHS of
tests/test_ode_train.py: an ensemble is exactly its members, bit for bit."""
import pytest
import torch

import kanode

from test_ode_train import lotka

PTRUE = torch.tensor([1.5, 1.0, 1.0, 3.0], dtype=torch.float64)
U0 = torch.tensor([1.0, 1.0], dtype=torch.float64)
TS = [0.1 * i for i in range(35)]
P0 = torch.stack([PTRUE * 1.1, PTRUE * 0.9, PTRUE * 1.05 + 0.01])
ETA = [1e-2, 5e-3, 2e-2]
LAM = [0.0, 5e-4, 1e-3]


@pytest.fixture(scope="module")
def target():
    return kanode.solve(lotka, U0, (0.0, 3.5), PTRUE, saveat=TS, opt=kanode.Tsit5Options(abstol=1e-10, reltol=1e-10)).u


def single(target, r):
    return kanode.Trainer(lotka, U0, (0.0, 3.5), TS, target, P0[r], eta=ETA[r], sparse_reg=LAM[r])


def opt_state(tr):
    m, v, bp = tr.opt.state[id(tr.p)]
    return m, v, list(bp)


def test_ensemble_equals_its_members(target):
    """run(2) of R = 3 replicas with distinct p0, eta and sparse_reg = three Trainers stepped twice: p, history, m,
    v and the running powers, bit for bit; member(r).run(1) then continues exactly as a third ensemble iteration."""
    ens = kanode.EnsembleTrainer(lotka, U0, (0.0, 3.5), TS, target, P0, eta=ETA, sparse_reg=LAM)
    out = ens.run(2)
    assert ens.last_run == "host" and out["iters_done"] == [2, 2, 2] and out["stop"] == ["ok"] * 3
    assert out["loss"].shape == (3, 2) and out["loss_test"] is None and ens.stopped == {}
    refs = [single(target, r) for r in range(3)]
    for r, ref in enumerate(refs):
        ls = [ref.step(), ref.step()]
        m, v, bp = opt_state(ref)
        assert torch.equal(ens.p[r], ref.p) and torch.equal(ens.m[r], m) and torch.equal(ens.v[r], v)
        assert ens.bp[r] == bp and ens.history[r] == ls == out["loss"][r].tolist()
    r_best, l_best = ens.best()
    assert l_best == min(h[-1] for h in ens.history) and ens.history[r_best][-1] == l_best
    members = [ens.member(r) for r in range(3)]
    before = ens.p.clone()
    third = [mb.run(1)["loss"][0].item() for mb in members]
    assert torch.equal(ens.p, before)                     # a member is a clone: the ensemble is not touched
    out3 = ens.run(1)
    for r, mb in enumerate(members):
        m, v, bp = opt_state(mb)
        assert out3["loss"][r, 0].item() == third[r] and mb.history == ens.history[r]
        assert torch.equal(ens.p[r], mb.p) and torch.equal(ens.m[r], m) and torch.equal(ens.v[r], v)
        assert ens.bp[r] == bp
        assert refs[r].step() == third[r] and torch.equal(refs[r].p, mb.p)


def test_argument_checks(target):
    with pytest.raises(ValueError, match=r"\[R, P\]"):
        kanode.EnsembleTrainer(lotka, U0, (0.0, 3.5), TS, target, P0[0])
    with pytest.raises(ValueError, match="eta"):
        kanode.EnsembleTrainer(lotka, U0, (0.0, 3.5), TS, target, P0, eta=[1e-2, 1e-3])
    with pytest.raises(ValueError, match="sparse_reg"):
        kanode.EnsembleTrainer(lotka, U0, (0.0, 3.5), TS, target, P0, sparse_reg=[0.0] * 4)
