"""The handle's option table (csrc/kanode_options.hpp: every option's default, range, refusal text; the read-only,
one-of-a-set and table-dependent rows; unknown ids) and largest_fitting, the training loops' capacity search:
tests/host/options_test.cpp, a stand-alone program that states the decision table with literal expected values, built
with AddressSanitizer and UBSan and run directly (nothing is preloaded and nothing of it is loaded into Python; the
sanitizer runtimes are linked statically).  Where no host compiler has the sanitizer runtimes the program is built
plain: its own bookkeeping still checks every row."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "options_test.cpp")
INCS = [os.path.join(ROOT, "kan-odes_amd", "csrc"), os.path.join(ROOT, "include")]


def _compilers():
    found = [shutil.which(c) for c in (os.environ.get("CXX") or "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++")]
    return [c for c in dict.fromkeys(found) if c]


def _build(exe, flag_sets):
    for cxx in _compilers():
        for flags in flag_sets:
            r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags,
                                *[a for inc in INCS for a in ("-I", inc)], SRC, "-o", exe],
                               capture_output=True, text=True)
            if r.returncode == 0:
                return cxx, r
    return None, r


def test_options_host_program(tmp_path):
    assert _compilers(), "no host C++ compiler found"
    exe = str(tmp_path / "options_test")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    # (the static runtimes are spelled differently by gcc and clang)
    cxx, r = _build(exe, [san + ["-static-libasan", "-static-libubsan"], san + ["-static-libsan"]])
    if cxx is None:
        print("no compiler links the sanitizer runtimes; building plain:\n" + r.stderr[-2000:])
        cxx, r = _build(exe, [[]])
    assert cxx is not None, r.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "options_test ok" in run.stdout
