"""The seating order of the main pass (dhr_amd/csrc/seating.h) on the CPU: tests/seating_check.cpp includes that header alone and asserts that
the slots are a permutation in the documented order (longer bound lists first, ties by query number, padded queries in place behind the real
ones) -- built with AddressSanitizer and UBSan and run as a plain executable, as tests/test_search_plan.py does for the search plan."""
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
    raise AssertionError("no C++ compiler found for the stand-alone seating check")


def test_seating_order_invariants(tmp_path):
    exe = str(tmp_path / "seating_check")
    cxx = _compiler()
    # the sanitizer runtimes linked into the executable (clang's default): it runs whatever else the process environment loads first
    static_rt = [] if "clang" in os.path.basename(os.path.realpath(cxx)) else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static_rt + [
        "-I", CSRC, os.path.join(HERE, "seating_check.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert run.stdout.startswith("seating ok:"), run.stdout
    print(run.stdout.strip())
