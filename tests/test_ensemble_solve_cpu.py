"""The ensemble solve without a GPU: its C-ABI surface (kanode_solve_ensemble_tsit5,
kanode_solve_ensemble_supported) and the host path of kanode.solve_ensemble / EnsembleTrainer.predict / eval_loss,
the loop of solve() every RHS takes that the one-launch entry does not cover.

The problem is shape S1 of tests/test_gpu_train_wg.py ([2,4,2] tanh_fast, G = 5) on the CPU oracle's RHS.  The
maxiters case: over (0, 3.5) at the default tolerances `p` takes 6 iterations and `3p` takes 26 (22 accepted + 4
rejected), so maxiters = 12 separates them with a wide margin on either side."""
import math
import os
import re
import subprocess

import numpy as np
import torch

from conftest import ROOT
from test_gpu_train_wg import TS, data, specs_of

import kanode
from kanode import _lib as L
from oracle.oracle_rhs import OracleChainRHS

HEADER = os.path.join(ROOT, "include", "kanode.h")
ENTRIES = ["kanode_solve_ensemble_supported", "kanode_solve_ensemble_tsit5"]
# the export set tests/test_train_wg_cpu.py pins
TRAIN_ENTRIES = ["kanode_train_ensemble_tsit5", "kanode_train_forward_ensemble_tsit5", "kanode_train_forward_supported",
                 "kanode_train_forward_tsit5", "kanode_train_supported", "kanode_train_tsit5"]


def problem(scales):
    p, u0, X = data("S1")
    ps = torch.as_tensor(np.stack([s * p for s in scales]))
    return OracleChainRHS(specs_of("S1")), torch.as_tensor(u0), ps, torch.as_tensor(X)


def test_header_binding_and_exports():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", src), name
    assert re.search(r"KANODE_SOLVE_OK\s*=\s*0\s*,\s*KANODE_SOLVE_MAXITERS\s*=\s*1\s*\}\s*kanode_solve_stop;", src)
    names = [n for n, _, _ in L.SIGNATURES]
    assert all(n in names for n in ENTRIES)
    # the header's argument count
    decl = re.search(r"kanode_solve_ensemble_tsit5\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
    sig = {n: a for n, _, a in L.SIGNATURES}
    assert len(decl.split(",")) == len(sig["kanode_solve_ensemble_tsit5"]) == 14
    assert L.SOLVE_STOP == {0: "ok", 1: "maxiters"}
    out = subprocess.run(["nm", "-D", "--defined-only", kanode.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\sT\s+(kanode_\w+)", out))
    assert set(ENTRIES) <= exported
    assert sorted(n for n in exported if "train" in n) == TRAIN_ENTRIES     # no exported name gained `train`
    assert not [n for n in ENTRIES if "train" in n or "_wg" in n or "any_chain" in n]
    # and the ensemble solve has no handle option of its own (21 = TRAIN_ANY_CHAIN, 22 = the read-only LAST_EVAL)
    assert max(L.OPTIONS.values()) == 22 and not [n for n in L.OPTIONS if "ensemble" in n]
    assert kanode.lib().kanode_solve_ensemble_supported(None, 1) == 0
    assert kanode.lib().kanode_solve_ensemble_tsit5(None, 1, None, None, 1, 0.0, 1.0, None, 0, None, None, None, None,
                                                    None) == L.ERR_INVALID_ARG


def test_host_path_equals_the_loop_of_solve():
    f, u0, ps, _ = problem([1.0, 0.5, 2.0])
    for opt in (kanode.Tsit5Options(), kanode.Tsit5Options(adaptive=False, dt=0.01)):
        ens = kanode.solve_ensemble(f, u0, (0.0, 3.5), ps, TS, opt)
        assert isinstance(ens, kanode.EnsembleSolution) and ens.path == "host" and ens.stop == ["ok"] * 3
        assert ens.t == TS and ens.u.shape == (3, 35, 1, 2) and not ens.u.requires_grad
        for r in range(3):
            one = kanode.solve(f, u0, (0.0, 3.5), ps[r], TS, opt)
            assert torch.equal(ens.u[r], one.u) and ens.stats[r] == one.stats
        assert not torch.equal(ens.u[0], ens.u[1])
    # inputs that carry gradients are detached, and a saveat of None is solve()'s [t0, tf]
    ens = kanode.solve_ensemble(f, u0.clone().requires_grad_(), (0.0, 1.0), ps.clone().requires_grad_())
    assert ens.t == [0.0, 1.0] and ens.u.shape == (3, 2, 1, 2) and not ens.u.requires_grad


def test_host_path_maxiters_stops_one_replica():
    f, u0, ps, _ = problem([1.0, 3.0, 1.0])
    free = kanode.Tsit5Options()
    its = [(s["naccept"] + s["nreject"]) for s in kanode.solve_ensemble(f, u0, (0.0, 3.5), ps, TS, free).stats]
    print("iterations", its)
    assert its[0] < 12 < its[1]
    opt = kanode.Tsit5Options(maxiters=12)
    ens = kanode.solve_ensemble(f, u0, (0.0, 3.5), ps, TS, opt)
    assert ens.stop == ["ok", "maxiters", "ok"] and ens.path == "host"
    assert torch.isnan(ens.u[1]).all()
    one = kanode.solve(f, u0, (0.0, 3.5), ps[0], TS, opt)
    for r in (0, 2):
        assert torch.equal(ens.u[r], one.u) and ens.stats[r] == one.stats


def test_ensemble_trainer_predict_and_eval_loss_on_the_cpu():
    f, u0, ps, X = problem([1.0, 0.5, 2.0])
    ens = kanode.EnsembleTrainer(f, u0, (0.0, 3.5), TS, X, ps, eta=1e-3)
    ens.run(1)
    before = (ens.p.clone(), ens.m.clone(), ens.v.clone(), [list(b) for b in ens.bp], [list(h) for h in ens.history],
              [tr._pver for tr in ens._members], [tr._pre for tr in ens._members])
    assert ens.last_predict is None
    sol = ens.predict()
    assert ens.last_predict == "host" and sol.path == "host" and sol.u.shape == (3, 35, 1, 2)
    losses = ens.eval_loss()
    ts_t = [0.1 * i for i in range(41)]
    X_t = torch.as_tensor(np.random.default_rng(12).uniform(0.5, 2.0, (41, 1, 2)))
    losses_t = ens.eval_loss(test=((0.0, 4.0), ts_t, X_t))
    assert isinstance(losses, list) and len(losses) == 3 and all(math.isfinite(x) for x in losses + losses_t)
    for r in range(3):
        m = ens.member(r)
        that = m.predict(m.p).u
        assert torch.equal(sol.u[r], that)
        assert losses[r] == float(kanode.mse_loss(that, X))
        that_t = kanode.solve(f, u0, (0.0, 4.0), m.p, ts_t, m.solver).u
        assert losses_t[r] == float(kanode.mse_loss(that_t, X_t))
    after = (ens.p, ens.m, ens.v, [list(b) for b in ens.bp], [list(h) for h in ens.history],
             [tr._pver for tr in ens._members], [tr._pre for tr in ens._members])
    assert all(torch.equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3:] == after[3:]
