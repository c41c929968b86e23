"""The sharded step's plan (dhr_amd/csrc/sharded_plan.h) on the CPU: tests/sharded_plan_check.cpp includes that header alone and checks, over a
grid of batch sizes, k, world sizes 1..70 and ranks, the block layouts (aligned payloads and strides, ordered list sections), prefix_len, the
rank vote (pack -> reduce -> unpack against a plain restatement) and the order of the planned all-gathers -- built with AddressSanitizer and
UBSan and run as a plain executable."""
import os
import subprocess

from tests.test_search_plan import _compiler

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "dhr_amd", "csrc")


def test_sharded_plan_invariants(tmp_path):
    exe = str(tmp_path / "sharded_plan_check")
    cxx = _compiler()
    # the sanitizer runtimes linked into the executable (clang's default): it runs whatever else the process environment loads first
    static_rt = [] if "clang" in os.path.basename(os.path.realpath(cxx)) else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static_rt + [
        "-I", CSRC, os.path.join(HERE, "sharded_plan_check.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert run.stdout.startswith("sharded plan ok:"), run.stdout
    print(run.stdout.strip())
