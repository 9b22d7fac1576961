"""The trajectory ensemble without a GPU: its C-ABI surface (kanode_solve_trajectories_tsit5,
kanode_solve_trajectories_supported) and the host path of kanode.solve_trajectories, the loop of solve() at batch 1
that every RHS takes which the one-launch entry does not cover.

The problem is shape S1 of tests/test_gpu_train_wg.py ([2,4,2] tanh_fast, G = 5) on the CPU oracle's RHS at
p = 3·data("S1")[0], from nine initial conditions default_rng(21).uniform(0.5, 2.0, (9, 2)) over (0, 3.5).  At the
default tolerances the batched solve of the nine takes 24 steps and the nine solves on their own 19 to 22 accepted
steps, six of them with at least one rejection.  The maxiters case: rows 1 and 6 scaled by 8 need 3 iterations, the
others at least 19, so maxiters = 12 separates them with a wide margin on either side."""
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
ENTRIES = ["kanode_solve_trajectories_supported", "kanode_solve_trajectories_tsit5"]
# the export set tests/test_train_wg_cpu.py pins
TRAIN_ENTRIES = ["kanode_train_ensemble_tsit5", "kanode_train_forward_ensemble_tsit5", "kanode_train_forward_supported",
                 "kanode_train_forward_tsit5", "kanode_train_supported", "kanode_train_tsit5"]
_REF = {}


def problem():
    p = 3.0 * data("S1")[0]
    u0 = np.random.default_rng(21).uniform(0.5, 2.0, (9, 2))
    return OracleChainRHS(specs_of("S1")), torch.as_tensor(u0), torch.as_tensor(p)


def loop_of_solve(key, f, u0, p, opt):
    """kanode.solve at every row of u0 on its own (computed once per key)."""
    if key not in _REF:
        _REF[key] = [kanode.solve(f, u0[r:r + 1], (0.0, 3.5), p, TS, opt) for r in range(u0.shape[0])]
    return _REF[key]


def test_header_binding_and_exports():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", src), name
    names = [n for n, _, _ in L.SIGNATURES]
    assert all(n in names for n in ENTRIES)
    # the header's argument counts
    sig = {n: a for n, _, a in L.SIGNATURES}
    decl = re.search(r"kanode_solve_trajectories_tsit5\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
    assert len(decl.split(",")) == len(sig["kanode_solve_trajectories_tsit5"]) == 13
    decl = re.search(r"kanode_solve_trajectories_supported\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
    assert len(decl.split(",")) == len(sig["kanode_solve_trajectories_supported"]) == 1
    out = subprocess.run(["nm", "-D", "--defined-only", kanode.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\sT\s+(kanode_\w+)", out))
    assert set(ENTRIES) <= exported
    assert sorted(n for n in exported if "train" in n) == TRAIN_ENTRIES     # no exported name gained `train`
    assert not [n for n in ENTRIES if "train" in n or "_wg" in n or "any_chain" in n or "fit_ensemble" in n]
    # and the trajectory solve has no handle option of its own (22 = the read-only LAST_EVAL)
    assert max(L.OPTIONS.values()) == 22 and not [n for n in L.OPTIONS if "traj" in n]


def test_null_handle_returns():
    assert kanode.lib().kanode_solve_trajectories_supported(None) == 0
    assert kanode.lib().kanode_solve_trajectories_tsit5(None, None, None, 1, 0.0, 1.0, None, 0, None, None, None, None,
                                                        None) == L.ERR_INVALID_ARG


def test_host_path_equals_the_loop_of_solve():
    f, u0, p = problem()
    for key, opt in (("default", kanode.Tsit5Options()), ("fixed", kanode.Tsit5Options(adaptive=False, dt=0.01))):
        ens = kanode.solve_trajectories(f, u0, (0.0, 3.5), p, TS, opt)
        assert isinstance(ens, kanode.TrajectorySolution) and ens.path == "host" and ens.stop == ["ok"] * 9
        assert ens.t == TS and ens.u.shape == (35, 9, 2) and not ens.u.requires_grad
        for r, one in enumerate(loop_of_solve(key, f, u0, p, opt)):
            assert torch.equal(ens.u[:, r:r + 1, :], one.u) and ens.stats[r] == one.stats
        assert not torch.equal(ens.u[:, 0], ens.u[:, 1])


def test_every_trajectory_has_its_own_step_control():
    """The nine solves differ from the batched solve of the same u0, which is ONE ODE: 24 steps there, 19 to 22
    accepted steps here (19, 19, 22, 19, 20, 21, 19, 19, 20), six of them with a rejected step and three without."""
    f, u0, p = problem()
    ens = kanode.solve_trajectories(f, u0, (0.0, 3.5), p, TS)
    batched = kanode.solve(f, u0, (0.0, 3.5), p, TS)
    nacc = [s["naccept"] for s in ens.stats]
    nrej = [s["nreject"] for s in ens.stats]
    print("naccept", nacc, "nreject", nrej, "batched", batched.stats)
    assert batched.stats["naccept"] == 24
    assert min(nacc) == 19 and max(nacc) == 22
    assert len(set(nacc)) >= 2 and any(x > 0 for x in nrej) and any(x == 0 for x in nrej)
    assert ens.u.shape == batched.u.shape and not torch.equal(ens.u, batched.u)


def test_inputs_are_detached_and_saveat_defaults_to_the_span():
    f, u0, p = problem()
    ens = kanode.solve_trajectories(f, u0[:3].clone().requires_grad_(), (0.0, 1.0), p.clone().requires_grad_())
    assert ens.t == [0.0, 1.0] and ens.u.shape == (2, 3, 2) and not ens.u.requires_grad
    try:
        kanode.solve_trajectories(f, u0[0], (0.0, 1.0), p)
    except ValueError as e:
        assert "[R, N]" in str(e)
    else:
        raise AssertionError("a vector u0 was accepted")


def test_host_path_maxiters_stops_trajectories_alone():
    f, u0, p = problem()
    u0 = u0.clone()
    u0[[1, 6]] *= 8.0
    free = kanode.solve_trajectories(f, u0, (0.0, 3.5), p, TS)
    its = [s["naccept"] + s["nreject"] for s in free.stats]
    print("iterations", its)
    assert its[1] == 3 and its[6] == 3 and min(x for r, x in enumerate(its) if r not in (1, 6)) >= 19
    opt = kanode.Tsit5Options(maxiters=12)
    ens = kanode.solve_trajectories(f, u0, (0.0, 3.5), p, TS, opt)
    assert ens.path == "host" and ens.stop == ["ok" if r in (1, 6) else "maxiters" for r in range(9)]
    for r in range(9):
        if r in (1, 6):
            one = kanode.solve(f, u0[r:r + 1], (0.0, 3.5), p, TS, opt)
            assert torch.equal(ens.u[:, r:r + 1, :], one.u) and ens.stats[r] == one.stats
        else:
            assert torch.isnan(ens.u[:, r]).all()
