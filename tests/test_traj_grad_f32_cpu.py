"""The fp32 trajectory-ensemble gradient without a GPU: its C-ABI surface (kanode_trajectories_gradient_f32_supported,
_group, _tsit5), the Python names and the f32 keyword, the float32 summation order of the reduction, and the fall-back
of f32="device" to the host path where no handle covers the problem.

The problem of the last test is tests/test_traj_grad_cpu.py's (shape S1 on the CPU oracle's RHS) with float32 p."""
import inspect
import re
import subprocess

import numpy as np
import torch

from test_gpu_train_wg import TS, data, specs_of
from test_traj_grad_cpu import HEADER

import kanode
from kanode import _lib as L
from kanode.adjoint import combine_trajectory_rows
from oracle.oracle_rhs import OracleChainRHS

ENTRIES = {"kanode_trajectories_gradient_f32_supported": 1, "kanode_trajectories_gradient_f32_group": 5,
           "kanode_trajectories_gradient_f32_tsit5": 20}


def chunk_order_mean_f32(rows):
    """The reduction's order in float32 arithmetic: chunks of 64 consecutive rows summed from 0.0f in ascending r, the
    chunk sums from 0.0f in ascending chunk order, one division by float32(R); every operation rounded to float32."""
    rows = np.asarray(rows)
    assert rows.dtype == np.float32
    R = rows.shape[0]
    tot = np.zeros(rows.shape[1], dtype=np.float32)
    for c0 in range(0, R, 64):
        s = np.zeros(rows.shape[1], dtype=np.float32)
        for r in range(c0, min(R, c0 + 64)):
            s = s + rows[r]
        tot = tot + s
    out = tot / np.float32(R)
    assert out.dtype == np.float32
    return out


def test_header_binding_and_exports():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    sig = {n: a for n, _, a in L.SIGNATURES}
    ret = {n: r for n, r, _ in L.SIGNATURES}
    for name, nargs in ENTRIES.items():
        decl = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(sig[name]) == nargs, name
        # argument for argument the fp64 entry's binding
        twin = name.replace("_f32", "")
        assert sig[name] == sig[twin] and ret[name] == ret[twin], name
    out = subprocess.run(["nm", "-D", "--defined-only", kanode.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\sT\s+(kanode_\w+)", out))
    assert set(ENTRIES) <= exported
    # no handle option of its own (22 = the read-only LAST_EVAL)
    assert max(L.OPTIONS.values()) == 22 and not [n for n in L.OPTIONS if "traj" in n]
    # the fp64 entry's comment still says that the L1 penalty is not read, and points to the new entries
    text = open(HEADER).read()
    assert re.search(r"does NOT read the handle's\s+\*?\s*L1 penalty", text)
    fp64_comment = text[:text.index("int32_t kanode_trajectories_gradient_supported")]
    assert "kanode_trajectories_gradient_f32_tsit5" in fp64_comment


def test_null_handle_returns():
    lib = kanode.lib()
    assert lib.kanode_trajectories_gradient_f32_supported(None) == 0
    assert lib.kanode_trajectories_gradient_f32_group(None, 0.0, 1.0, 1, None) == 0
    assert lib.kanode_trajectories_gradient_f32_tsit5(None, None, None, 1, 0.0, 1.0, None, 0, None, None, None, None,
                                                      None, None, None, None, None, None, None,
                                                      None) == L.ERR_INVALID_ARG


def test_python_names_and_the_f32_keyword():
    for m in ("trajectories_gradient_f32_supported", "trajectories_gradient_f32_group",
              "trajectories_gradient_f32_tsit5"):
        assert callable(getattr(kanode.KanodeHandle, m))
    assert inspect.signature(kanode.trajectories_mse_gradient).parameters["f32"].default == "host"
    assert inspect.signature(kanode.TrajectoryTrainer.__init__).parameters["f32"].default == "host"
    # the two methods take the same arguments
    a = inspect.signature(kanode.KanodeHandle.trajectories_gradient_tsit5)
    b = inspect.signature(kanode.KanodeHandle.trajectories_gradient_f32_tsit5)
    assert list(a.parameters) == list(b.parameters)
    assert not hasattr(kanode.TrajectoryTrainer, "dp_group")


def test_float32_summation_order():
    """The float32 restatement and kanode's torch statement of the order agree bitwise on float32 rows at R = 1, 63,
    64, 65 and 1030; only at 1030 does the chunked result differ from the plain ascending float32 sum."""
    rng = np.random.default_rng(3)
    for R in (1, 63, 64, 65, 1030):
        rows = (rng.normal(size=(R, 7)) * 10.0 ** rng.integers(-3, 4, size=(R, 1))).astype(np.float32)
        want = chunk_order_mean_f32(rows)
        got = combine_trajectory_rows(torch.as_tensor(rows))
        assert got.dtype == torch.float32
        assert np.array_equal(got.numpy(), want), R
        naive = np.zeros(7, dtype=np.float32)
        for r in range(R):
            naive = naive + rows[r]
        naive = naive / np.float32(R)
        print(R, "chunked vs ascending float32 sum", np.abs(want - naive).max())
        assert np.array_equal(want, naive) == (R != 1030), R


def test_f32_device_falls_back_to_the_host_path_on_the_cpu():
    """OracleChainRHS has no handle: f32="device" takes the host path, with the results of the default call."""
    f = OracleChainRHS(specs_of("S1"))
    p = torch.as_tensor(3.0 * data("S1")[0]).to(torch.float32)
    u0 = torch.as_tensor(np.random.default_rng(21).uniform(0.5, 2.0, (9, 2)))[:3].to(torch.float32).contiguous()
    X = torch.as_tensor(np.random.default_rng(5).uniform(0.5, 2, (35, 9, 2)))[:, :3].to(torch.float32).contiguous()
    opt = kanode.Tsit5Options(adaptive=False, dt=0.05)
    l0, g0, i0 = kanode.trajectories_mse_gradient(f, u0, (0.0, 3.5), p, TS, X, opt, rows=True)
    l1, g1, i1 = kanode.trajectories_mse_gradient(f, u0, (0.0, 3.5), p, TS, X, opt, rows=True, f32="device")
    assert i0["path"] == i1["path"] == "host" and i1["stop"] == ["ok"] * 3
    assert g1.dtype == torch.float32 and l0 == l1 and torch.equal(g0, g1)
    assert torch.equal(i0["dp_rows"], i1["dp_rows"]) and torch.equal(i0["loss_rows"], i1["loss_rows"])
    rows = np.concatenate([i1["dp_rows"].numpy(), i1["loss_rows"].numpy()[:, None]], axis=1)
    want = chunk_order_mean_f32(rows)
    assert np.array_equal(g1.numpy(), want[:-1]) and l1 == float(want[-1])
    tr = kanode.TrajectoryTrainer(f, u0, (0.0, 3.5), TS, X, p, solver=opt, f32="device")
    lt, gt, it = tr.loss_and_grad()
    assert it["path"] == "host" and torch.equal(gt, g0) and float(lt) == l0
    try:
        kanode.trajectories_mse_gradient(f, u0, (0.0, 3.5), p, TS, X, opt, f32="gpu")
    except ValueError as e:
        assert "f32" in str(e)
    else:
        raise AssertionError("an unknown f32 value was accepted")
