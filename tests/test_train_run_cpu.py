"""Trainer.run without a GPU: the step() loop it falls back to for every RHS the device-resident loop does not
cover, and the C-ABI surface of that loop (kanode_train_tsit5, kanode_train_supported)."""
import re
import subprocess

import numpy as np
import torch

import kanode
from kanode import _lib as L
from oracle import oracle as O
from oracle.oracle_rhs import OracleChainRHS

SPECS = [O.LayerSpec(2, 10, 5, "tanh_fast"), O.LayerSpec(10, 2, 5, "tanh_fast")]
TS = [0.1 * i for i in range(11)]
TS_TEST = [0.1 * i for i in range(21)]


def trainer():
    f = OracleChainRHS(SPECS)
    u0 = torch.tensor([[1.0, 1.0]], dtype=torch.float64)
    p0 = torch.as_tensor(np.random.default_rng(5).uniform(-0.1, 0.1, 240))
    target = torch.as_tensor(np.random.default_rng(6).uniform(0.5, 2.0, (11, 1, 2)))
    return f, u0, kanode.Trainer(f, u0, (0.0, 1.0), TS, target, p0, eta=1e-2)


def test_run_equals_the_step_loop_on_a_cpu_rhs():
    f, u0, a = trainer()
    _, _, b = trainer()
    target_t = torch.as_tensor(np.random.default_rng(7).uniform(0.5, 2.0, (21, 1, 2)))
    out = a.run(3, test=((0.0, 2.0), TS_TEST, target_t), record=True)
    ls, lt, pbs = [], [], []
    for _ in range(3):
        pbs.append(b.p.clone())
        ls.append(b.step())
        with torch.no_grad():
            lt.append(float(kanode.mse_loss(kanode.solve(f, u0, (0.0, 2.0), b.p, TS_TEST, b.solver).u, target_t)))
    assert torch.equal(a.p, b.p) and a.history == b.history == ls
    assert sorted(out) == ["counts", "grad", "loss", "loss_test", "p_before"]
    assert out["loss"].tolist() == ls and out["loss_test"].tolist() == lt
    assert out["loss"].dtype == torch.float64 and out["loss"].shape == (3,) and out["loss_test"].shape == (3,)
    assert out["grad"].shape == (3, 240) and out["p_before"].shape == (3, 240) and out["counts"].shape == (3, 4)
    assert torch.equal(out["p_before"], torch.stack(pbs))
    assert (out["counts"][:, 0] > 0).all() and (out["counts"][:, 2] > 0).all()
    # the recorded gradient is the one the update used
    _, _, c = trainer()
    for it in range(3):
        assert torch.equal(c.p, out["p_before"][it])
        c.opt.update(c.p, out["grad"][it])
    assert torch.equal(c.p, a.p)
    plain = trainer()[2].run(2)
    assert sorted(plain) == ["loss", "loss_test"] and plain["loss_test"] is None and plain["loss"].tolist() == ls[:2]
    assert trainer()[2].run(0)["loss"].shape == (0,)


def test_run_drops_the_cached_forward():
    """A run advances _pver by its iterations and leaves no cached forward of eval_loss behind: loss_and_grad()
    after it is that of a fresh Trainer at the same p."""
    _, _, tr = trainer()
    tr.eval_loss()
    tr._pre = (tr._pver, "stale", "a stale forward")  # (a CPU RHS keeps none itself: plant one)
    tr.run(2)
    assert tr._pre is None and tr._pver == 2 and len(tr.history) == 2
    loss, g, _ = tr.loss_and_grad()
    _, _, fresh = trainer()
    fresh.p = tr.p.clone()
    l2, g2, _ = fresh.loss_and_grad()
    assert float(loss) == float(l2) and torch.equal(g, g2)


def test_library_exports_the_training_entries():
    out = subprocess.run(["nm", "-D", "--defined-only", kanode.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\sT\s+(kanode_\w+)", out))
    assert {"kanode_train_tsit5", "kanode_train_supported"} <= exported
    names = [n for n, _, _ in L.SIGNATURES]
    assert "kanode_train_tsit5" in names and "kanode_train_supported" in names
    assert kanode.lib().kanode_abi_version() == 1
    assert kanode.lib().kanode_train_supported(None, 1) == 0
