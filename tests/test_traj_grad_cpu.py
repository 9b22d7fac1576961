"""The trajectory-ensemble gradient without a GPU: its C-ABI surface (kanode_trajectories_gradient_supported, _group,
_tsit5), the Python names, the summation order of the reduction and the host path of kanode.trajectories_mse_gradient
(a loop of batch-1 gradients combined in the device's order).

The problem is shape S1 of tests/test_gpu_train_wg.py on the CPU oracle's RHS at p = 3·data("S1")[0], from the first
five of the nine initial conditions default_rng(21).uniform(0.5, 2.0, (9, 2)) over (0, 3.5) at dt = 0.01, against
default_rng(5).uniform(0.5, 2, (35, 9, 2))."""
import os
import re
import subprocess

import numpy as np
import torch

from conftest import ROOT
from test_gpu_train_wg import TS, data, specs_of
from test_host_traj_grad import build_program

import kanode
from kanode import _lib as L
from kanode.adjoint import combine_trajectory_rows
from oracle.oracle_rhs import OracleChainRHS

HEADER = os.path.join(ROOT, "include", "kanode.h")
ENTRIES = {"kanode_trajectories_gradient_supported": 1, "kanode_trajectories_gradient_group": 5,
           "kanode_trajectories_gradient_tsit5": 20}


def chunk_order_mean(rows):
    """The reduction's order restated in numpy: chunks of 64 consecutive rows summed from 0.0 in ascending r, the
    chunk sums from 0.0 in ascending chunk order, one division by R."""
    rows = np.asarray(rows, dtype=np.float64)
    R = rows.shape[0]
    tot = np.zeros(rows.shape[1])
    for c0 in range(0, R, 64):
        s = np.zeros(rows.shape[1])
        for r in range(c0, min(R, c0 + 64)):
            s = s + rows[r]
        tot = tot + s
    return tot / np.float64(R)


def test_header_binding_and_exports():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    sig = {n: a for n, _, a in L.SIGNATURES}
    for name, nargs in ENTRIES.items():
        decl = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(sig[name]) == nargs, name
    out = subprocess.run(["nm", "-D", "--defined-only", kanode.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\sT\s+(kanode_\w+)", out))
    assert set(ENTRIES) <= exported
    # no handle option of its own (22 = the read-only LAST_EVAL)
    assert max(L.OPTIONS.values()) == 22 and not [n for n in L.OPTIONS if "traj" in n]
    # the header says that the L1 penalty is not read
    assert re.search(r"does NOT read the handle's\s+\*?\s*L1 penalty", open(HEADER).read())


def test_python_names():
    assert "trajectories_mse_gradient" in kanode.__all__ and "TrajectoryTrainer" in kanode.__all__
    for m in ("trajectories_gradient_supported", "trajectories_gradient_group", "trajectories_gradient_tsit5"):
        assert callable(getattr(kanode.KanodeHandle, m))
    for m in ("loss_and_grad", "step", "run", "predict"):
        assert callable(getattr(kanode.TrajectoryTrainer, m))
    assert not hasattr(kanode.TrajectoryTrainer, "dp_group")


def test_null_handle_returns():
    lib = kanode.lib()
    assert lib.kanode_trajectories_gradient_supported(None) == 0
    assert lib.kanode_trajectories_gradient_group(None, 0.0, 1.0, 1, None) == 0
    assert lib.kanode_trajectories_gradient_tsit5(None, None, None, 1, 0.0, 1.0, None, 0, None, None, None, None, None,
                                                  None, None, None, None, None, None, None) == L.ERR_INVALID_ARG


def test_summation_order_matches_the_host_program(tmp_path):
    """The chunk bounds tests/host/traj_grad_args_test.cpp prints from kan_ensemble.hpp's functions are those of the
    numpy restatement, and the restatement and kanode's torch statement of the order agree bitwise on random rows, at
    R = 1, 63, 64, 65 and 1030; at 1030 the result is not the plain ascending sum's."""
    exe = str(tmp_path / "traj_grad_args_test")
    build_program(exe)
    rng = np.random.default_rng(3)
    for R in (1, 63, 64, 65, 1030):
        out = subprocess.run([exe, "chunks", str(R)], capture_output=True, text=True, timeout=60, check=True).stdout
        bounds = [tuple(int(x) for x in line.split()) for line in out.strip().splitlines()]
        assert bounds == [(c0, min(R, c0 + 64)) for c0 in range(0, R, 64)], R
        rows = rng.normal(size=(R, 7)) * 10.0 ** rng.integers(-3, 4, size=(R, 1))
        want = chunk_order_mean(rows)
        # the same order spelled with the program's bounds
        tot = np.zeros(7)
        for b, e in bounds:
            s = np.zeros(7)
            for r in range(b, e):
                s = s + rows[r]
            tot = tot + s
        assert np.array_equal(tot / np.float64(R), want)
        got = combine_trajectory_rows(torch.as_tensor(rows)).numpy()
        assert np.array_equal(got, want), R
        naive = np.zeros(7)
        for r in range(R):
            naive = naive + rows[r]
        print(R, "chunked vs ascending sum", np.abs(want - naive / R).max())
        if R == 1030:
            assert not np.array_equal(want, naive / R)


def test_host_path_is_the_chunk_ordered_mean_of_batch_1_gradients():
    f = OracleChainRHS(specs_of("S1"))
    p = torch.as_tensor(3.0 * data("S1")[0])
    u0 = torch.as_tensor(np.random.default_rng(21).uniform(0.5, 2.0, (9, 2)))[:5].contiguous()
    X = torch.as_tensor(np.random.default_rng(5).uniform(0.5, 2, (35, 9, 2)))[:, :5].contiguous()
    opt = kanode.Tsit5Options(adaptive=False, dt=0.01)
    loss, dp, info = kanode.trajectories_mse_gradient(f, u0, (0.0, 3.5), p, TS, X, opt, rows=True)
    assert info["path"] == "host" and info["stop"] == ["ok"] * 5
    assert isinstance(loss, float) and dp.shape == p.shape and info["dp_rows"].shape == (5, p.numel())
    rows = []
    for r in range(5):
        pr = p.clone().requires_grad_(True)
        sol = kanode.solve(f, u0[r:r + 1], (0.0, 3.5), pr, TS, opt)
        lr = kanode.mse_loss(sol.u, X[:, r:r + 1])
        (g,) = torch.autograd.grad(lr, pr)
        assert torch.equal(info["dp_rows"][r], g) and float(info["loss_rows"][r]) == float(lr.detach())
        assert info["fwd_stats"][r]["naccept"] == 350
        rows.append(np.concatenate([g.numpy(), [float(lr.detach())]]))
    want = chunk_order_mean(np.stack(rows))
    assert np.array_equal(dp.numpy(), want[:-1]) and loss == want[-1]
    # the total is mse_loss over the whole tensor up to summation order
    whole = float(kanode.mse_loss(kanode.solve_trajectories(f, u0, (0.0, 3.5), p, TS, opt).u, X))
    assert abs(loss - whole) <= 4 * X.numel() * 2.0 ** -53 * whole
    assert not torch.equal(info["dp_rows"][0], info["dp_rows"][1])


def test_trajectory_trainer_on_the_cpu_adds_the_l1_term_and_steps():
    f = OracleChainRHS(specs_of("S1"))
    p = torch.as_tensor(3.0 * data("S1")[0])
    u0 = torch.as_tensor(np.random.default_rng(21).uniform(0.5, 2.0, (9, 2)))[:2].contiguous()
    X = torch.as_tensor(np.random.default_rng(5).uniform(0.5, 2, (35, 9, 2)))[:, :2].contiguous()
    opt = kanode.Tsit5Options(adaptive=False, dt=0.05)
    plain = kanode.TrajectoryTrainer(f, u0, (0.0, 3.5), TS, X, p, eta=1e-3, solver=opt)
    reg = kanode.TrajectoryTrainer(f, u0, (0.0, 3.5), TS, X, p, eta=1e-3, solver=opt, sparse_reg=5e-4)
    l0, g0, _ = plain.loss_and_grad()
    l1, g1, _ = reg.loss_and_grad()
    assert torch.equal(l1, l0 + kanode.reg_loss(p, 5e-4, 0.0)) and torch.equal(g1, g0 + 5e-4 * torch.sign(p))
    out = plain.run(2, record=True)
    assert len(out["loss"]) == 2 and torch.equal(out["p_before"][0], p) and torch.equal(out["grad"][0], g0)
    ad = kanode.Adam(1e-3)
    x = p.clone()
    ad.update(x, g0)
    assert torch.equal(x, out["p_before"][1]) and plain.history == out["loss"]
    # maxiters on every trajectory: step() raises before the update
    stuck = kanode.TrajectoryTrainer(f, u0, (0.0, 3.5), TS, X, p, solver=kanode.Tsit5Options(maxiters=3))
    try:
        stuck.step()
    except L.KanodeError as e:
        assert "trajectory 0 stopped (forward_maxiters)" in str(e)
    else:
        raise AssertionError("a stopped trajectory did not raise")
    assert torch.equal(stuck.p, p) and not stuck.opt.state and stuck.history == []
