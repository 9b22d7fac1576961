"""The host code of a trajectory-ensemble gradient call (csrc/kan_ensemble.hpp: the buffer layout, the private
blocks, the group size and the summation order of the reduction): tests/host/traj_grad_args_test.cpp, a stand-alone
program, built with AddressSanitizer and UBSan and run directly (nothing is preloaded and nothing of it is loaded into
Python; the sanitizer runtimes are linked statically, so the program does not depend on what else the process loads
first).  Where no host compiler has the sanitizer runtimes the program is built plain: its own bookkeeping still checks
every property."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "traj_grad_args_test.cpp")
INC = os.path.join(ROOT, "kan-odes_amd", "csrc")


def _compilers():
    found = [shutil.which(c) for c in (os.environ.get("CXX") or "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++")]
    return [c for c in dict.fromkeys(found) if c]


def _build(exe, flag_sets):
    for cxx in _compilers():
        for flags in flag_sets:
            r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", INC, SRC, "-o", exe],
                               capture_output=True, text=True)
            if r.returncode == 0:
                return cxx, r
    return None, r


def build_program(exe):
    """The program at `exe`, with the sanitizers where a compiler links them; returns the compiler used."""
    assert _compilers(), "no host C++ compiler found"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    # (the static runtimes are spelled differently by gcc and clang)
    cxx, r = _build(exe, [san + ["-static-libasan", "-static-libubsan"], san + ["-static-libsan"]])
    if cxx is None:
        print("no compiler links the sanitizer runtimes; building plain:\n" + r.stderr[-2000:])
        cxx, r = _build(exe, [[]])
    assert cxx is not None, r.stderr[-4000:]
    return cxx


def test_traj_grad_args_host_program(tmp_path):
    exe = str(tmp_path / "traj_grad_args_test")
    build_program(exe)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "traj_grad_args_test ok" in run.stdout
