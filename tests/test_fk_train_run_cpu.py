"""The Fisher-KPP training loop without a GPU: the C-ABI surface of the device-resident loop on the forward-mode
gradient (kanode_train_forward_tsit5, kanode_train_forward_supported) and the host loop Trainer.run falls back to on
CPU tensors, which says so in last_run."""
import re
import subprocess

import numpy as np
import torch

import kanode
from kanode import _lib as L
from oracle import oracle as O
from oracle.oracle_rhs import OracleFKRHS

NX = 7
TS = [0.25 * i for i in range(5)]


def trainer():
    f = OracleFKRHS(O.LayerSpec(1, 1, 5, "tanh_fast"), 0.01, 1.0 / NX)
    rng = np.random.default_rng(8)
    x = np.arange(NX) / NX
    u0 = torch.as_tensor(np.exp(-((x - 0.5) / 0.2) ** 2)[None, :])
    p0 = torch.as_tensor(rng.normal(0.0, 0.3, 6))
    target = torch.as_tensor(rng.uniform(0.0, 1.0, (5, 1, NX)))
    return f, u0, target, kanode.Trainer(f, u0, (0.0, 1.0), TS, target, p0, eta=1e-2)


def test_library_exports_the_forward_training_entries():
    out = subprocess.run(["nm", "-D", "--defined-only", kanode.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\sT\s+(kanode_\w+)", out))
    assert {"kanode_train_forward_tsit5", "kanode_train_forward_supported"} <= exported
    names = [n for n, _, _ in L.SIGNATURES]
    assert "kanode_train_forward_tsit5" in names and "kanode_train_forward_supported" in names
    assert kanode.lib().kanode_train_forward_supported(None, 1, 0) == 0
    assert kanode.lib().kanode_train_forward_supported(None, 1, 1) == 0


def test_run_on_cpu_tensors_is_the_host_loop():
    f, u0, target, a = trainer()
    _, _, _, b = trainer()
    assert a.last_run is None
    out = a.run(2, test=((0.0, 1.0), TS, target))
    assert a.last_run == "host"
    ls, lt = [], []
    for _ in range(2):
        ls.append(b.step())
        with torch.no_grad():
            lt.append(float(kanode.mse_loss(kanode.solve(f, u0, (0.0, 1.0), b.p, TS, b.solver).u, target)))
    assert out["loss"].tolist() == ls and out["loss_test"].tolist() == lt
    assert torch.equal(a.p, b.p) and a.history == ls
