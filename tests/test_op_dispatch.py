"""The typed dispatch of the op launchers (dhr_amd/csrc/op_dispatch.h) on the CPU: tests/op_dispatch_check.cpp includes that header alone and asserts,
for every dispatcher and every code, that the lambda runs once with the expected type or constant, that its result comes back, that nested
dispatchers visit the full product and that a code outside a list runs no arm -- built as host C++ with AddressSanitizer and UBSan and run as a
plain executable.  _Float16 and __bf16 need clang."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "dhr_amd", "csrc")


def _compiler():
    path = shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    assert os.path.exists(path), "no clang++ found for the stand-alone dispatch check"
    return path


def test_op_dispatch_arms(tmp_path):
    exe = str(tmp_path / "op_dispatch_check")
    cmd = [_compiler(), "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(HERE, "op_dispatch_check.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert run.stdout.startswith("op dispatch ok:"), run.stdout
    assert int(run.stdout.split(":")[1].split()[0]) > 0, run.stdout
    print(run.stdout.strip())
