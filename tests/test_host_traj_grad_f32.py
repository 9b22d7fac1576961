"""The host code that plans an fp32 trajectory-ensemble gradient call (csrc/kan_ensemble.hpp: the element-size layout,
the float block and the group size; csrc/kan_chain_plan.hpp: the kernel's LDS carve and plan):
tests/host/traj_grad_f32_args_test.cpp, a stand-alone program, built with AddressSanitizer and UBSan and run directly,
the way tests/test_host_traj_grad.py builds and runs its program (nothing is preloaded and nothing of it is loaded
into Python)."""
import os
import subprocess

import test_host_traj_grad as H

SRC = os.path.join(H.ROOT, "tests", "host", "traj_grad_f32_args_test.cpp")


def test_traj_grad_f32_args_host_program(tmp_path, monkeypatch):
    monkeypatch.setattr(H, "SRC", SRC)
    exe = str(tmp_path / "traj_grad_f32_args_test")
    H.build_program(exe)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "traj_grad_f32_args_test ok" in run.stdout
