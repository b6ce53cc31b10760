"""The context's cache rules (csrc/factor_cache.hpp: adopt / known / forget / extend, the range
drop of a released workspace, the upper-only assembly's claim) checked on the CPU by a stand-alone
program: tests/host/factor_cache_check.cpp includes only that header, which includes nothing
from HIP.  Built with the host compiler, with AddressSanitizer and UBSan where they link, and
run directly (nothing is preloaded)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "factor_cache_check.cpp")
CSRC = os.path.join(HERE, "..", "gaussianprocessregression.jl_amd", "csrc")


def test_factor_cache_rules(tmp_path):
    cxx = os.environ.get("CXX") or next(filter(None, map(shutil.which, ("g++", "c++", "clang++"))),
                                        None)
    if not cxx:
        pytest.fail("no host C++ compiler found (g++, c++ or clang++)")
    exe = str(tmp_path / "factor_cache_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, SRC,
            "-o", exe]
    # (the runtimes linked statically, so the program does not depend on the order in which the
    # process loads its shared libraries; clang links them statically without being asked)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if "clang" not in os.path.basename(cxx):
        san += ["-static-libasan", "-static-libubsan"]
    built = subprocess.run(base + san, capture_output=True, text=True)
    if built.returncode != 0:  # the sanitizer runtimes do not link here: the plain build
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, plain.stderr
    print("sanitizers:", "address,undefined" if built.returncode == 0 else "none (did not link)")
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "factor cache rules ok" in run.stdout
