"""The search plan (dhr_amd/csrc/search_plan.h) on the CPU: tests/search_plan_check.cpp includes that header alone and asserts the plan's invariants
over a grid of corpus sizes, k, sample period / share, first rows, staged or not, depth 0 and 2 -- built with AddressSanitizer and UBSan
and run as a plain executable."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "dhr_amd", "csrc")


def _compiler():
    for cxx in ("g++", "clang++", "c++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path:
            return path
    raise AssertionError("no C++ compiler found for the stand-alone plan check")


def test_search_plan_invariants(tmp_path):
    exe = str(tmp_path / "search_plan_check")
    cxx = _compiler()
    # the sanitizer runtimes linked into the executable (clang's default): it runs whatever else the process environment loads first
    static_rt = [] if "clang" in os.path.basename(os.path.realpath(cxx)) else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra","-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static_rt + [
        "-I", CSRC, os.path.join(HERE, "search_plan_check.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert run.stdout.startswith("search plan ok:"), run.stdout
    print(run.stdout.strip())
