"""Forward sensitivities for fields of 65 to 128 entries: what can be checked without a GPU.

The option's place in the ABI, the CPU comparator of tests/test_gpu_fsens_wide.py pinned against the C port of the
same Dual solve (so that the GPU test's two references are known to agree with each other), and the host rule's
order: `forward_ok` turns `fsens_wide` on only after SciMLSensitivity's length(u0) + length(p) <= 100 rule passed."""
import os
import re

import numpy as np
import pytest
import torch

import fsens_restatement as R
from kanode import _lib as L
from kanode.adjoint import forward_ok
from kanode.ode import Tsit5Options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fsens_wide_option_is_20_in_binding_and_header():
    assert L.OPTIONS["fsens_wide"] == 20
    hdr = open(os.path.join(ROOT, "include", "kanode.h")).read()
    assert re.search(r"KANODE_OPT_FSENS_WIDE\s*=\s*20\b", hdr)
    # the option block documents it
    assert "KANODE_OPT_FSENS_WIDE (default 0)" in hdr


@pytest.mark.parametrize("tol,ubar,sbar", [(1e-3, 1e-6, 1e-6), (1e-6, 1e-9, 1e-8)])
@pytest.mark.parametrize("i", range(len(R.SHAPES)))
def test_restatement_matches_c_port_on_own_steps(i, tol, ubar, sbar):
    """The numpy restatement (oracle RHS / VJP + closed-form ∂φ/∂p) against the C port (dense Laplacian), each on
    its own steps: equal accepted / rejected counts (the recorded ones) and the GPU test's own-steps bars.  Measured:
    u within 9e-11 (1e-3) / 1e-12 (1e-6) of scale, every S_k within 6.6e-8 / 6e-11 of its own max."""
    pr = R.problem(*R.SHAPES[i])
    uc, Sc, stc = R.c_port(pr, tol)
    u, S, na, nr = R.restate(pr, Tsit5Options(abstol=tol * 1e-3, reltol=tol))
    eu, es = R.worst(u, S, uc, Sc)
    print(f"{R.SHAPES[i]} tol {tol}: C port {stc} restatement {na}/{nr} u {eu:.3g} S {es:.3g}")
    assert (na, nr) == (stc["naccept"], stc["nreject"]) == (R.COUNTS[tol][i], 0)
    assert eu <= ubar and es <= sbar


@pytest.mark.parametrize("Nx,B,G,dt,nrej", [c + (n,) for c, n in zip(R.FORCED, (2, 3, 2))])
def test_forced_first_steps_are_rejected_by_the_restatement(Nx, B, G, dt, nrej):
    """The inputs of the GPU test's reject-path cases: with this first step forced the controller rejects."""
    pr = R.problem(Nx, B, G)
    _, _, _, nr = R.restate(pr, Tsit5Options(dt=dt))
    assert nr == nrej


class _StubHandle:
    """Records what forward_ok asks of a handle."""

    def __init__(self):
        self.opts = {"fsens_wide": 0}
        self.calls = []

    def get_option(self, name):
        self.calls.append(("get", name))
        return self.opts[name]

    def set_option(self, name, value):
        self.calls.append(("set", name, value))
        self.opts[name] = value

    def forward_sensitivity_supported(self, batch):
        self.calls.append(("supported", batch, self.opts["fsens_wide"]))
        return True


class _StubRHS:
    auto_sensealg = True

    def __init__(self):
        self.hd = _StubHandle()


class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it lives on the device (forward_ok only looks at is_cuda, numel and shape)."""
    is_cuda = True


def _u0(B, Nx):
    return torch.zeros((B, Nx), dtype=torch.float64).as_subclass(_FakeCuda)


def test_forward_ok_turns_the_option_on_only_after_the_rule_passes():
    p = torch.zeros(11, dtype=torch.float64)
    # 90 + 11 = 101 > 100: the rule fails, and the handle is not touched
    f = _StubRHS()
    assert not forward_ok(f, _u0(1, 90), p)
    assert f.hd.calls == [] and f.hd.opts["fsens_wide"] == 0
    # 89 + 11 = 100: the option is on before the handle is asked
    f = _StubRHS()
    assert forward_ok(f, _u0(1, 89), p)
    assert f.hd.opts["fsens_wide"] == 1
    assert f.hd.calls[-1] == ("supported", 1, 1)
    assert ("set", "fsens_wide", 1) in f.hd.calls
    # idempotent: a second call sets nothing again and asks the same question
    n_set = sum(c[0] == "set" for c in f.hd.calls)
    assert forward_ok(f, _u0(1, 89), p)
    assert sum(c[0] == "set" for c in f.hd.calls) == n_set and f.hd.calls[-1] == ("supported", 1, 1)
    # a value the caller chose (2: the two-entry kernel everywhere) is kept
    f = _StubRHS()
    f.hd.opts["fsens_wide"] = 2
    assert forward_ok(f, _u0(3, 26), p)
    assert f.hd.opts["fsens_wide"] == 2 and f.hd.calls[-1] == ("supported", 3, 2)
    # not a hand-written ODEProblem (no automatic choice): untouched
    f = _StubRHS()
    f.auto_sensealg = False
    assert not forward_ok(f, _u0(1, 26), p) and f.hd.calls == []
