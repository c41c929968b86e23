"""The lexical heads after their host code moved onto one argument check, one workspace layout and one error style: what they answer to bad
arguments and what they compute, against tests/golden/lexical_entry_points.json and lexical_entry_points_gpu.json, which
tests/golden/make_golden_lexical_entry_points.py recorded at the commit before.  This module recomputes both with the recorder's own
functions.  The CPU half needs no device: every C case returns before the first HIP call -- (status, exact dhr_last_error text) --, the
workspace functions are host arithmetic, and every Python case raises before the library touches the device (exception type and text).
Cases named "beats" or "and" break two rules at once and pin which one answers.  The GPU half compares SHA-256 digests of every output:
the ops document bit-identical repeats, and two recordings at the parent agreed in every field.
dhr_amd/csrc/lexical_proj_layout.h is also checked on its own (tests/lexical_proj_layout_check.cpp, host C++ under ASan and UBSan)."""
import importlib.util
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "dhr_amd", "csrc")
ENTRY_POINTS = ("head_", "agg_", "train_", "back_", "proj_", "ptrain_", "pback_")


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_golden_lexical_entry_points", os.path.join(HERE, "golden", "make_golden_lexical_entry_points.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def pinned(gen):
    with open(gen.PATH_CHECKS) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got(gen):
    return gen.collect_checks()


def _differences(got, want):
    return {name: (got.get(name), v) for name, v in want.items() if got.get(name) != v}


def test_the_table_covers_every_entry_point(pinned):
    exits = pinned["exits"]
    for prefix in ENTRY_POINTS:
        assert sum(name.startswith(prefix) for name in exits) >= 20, prefix
        assert any(name.startswith(prefix) and "empty_batch" in name and v == [0, "bad argument"] for name, v in exits.items()), prefix
    assert sum("_beats_" in name or "_and_" in name for name in exits) >= 20
    assert {v[0] for v in exits.values()} == {0, -1, -2}          # DHR_OK, DHR_ERR_INVALID, DHR_ERR_UNSUPPORTED: no case reached a HIP call


def test_validation_exits_equal_the_parent(pinned, got):
    assert sorted(got["exits"]) == sorted(pinned["exits"])
    assert not _differences(got["exits"], pinned["exits"])


def test_workspace_sizes_equal_the_parent(gen, pinned, got):
    want = pinned["workspace"]
    n = len(gen.GRID_B) * len(gen.GRID_T) * len(gen.GRID_V)
    assert (len(want["head_train"]), len(want["proj"]), len(want["proj_train"])) == (n // len(gen.GRID_V), 4 * n, len(gen.GRID_H) * n)
    assert any(want["proj"]) and 0 in want["proj"] and any(want["proj_train"]) and 0 in want["proj_train"]
    assert got["workspace"] == want


def test_python_exits_equal_the_parent(pinned, got):
    want = pinned["python_exits"]
    assert len(want) >= 60 and all(kind != "no exception" for kind, _ in want.values())
    for module in ("lexical_", "proj_", "train_", "ptrain_"):
        assert any(name.startswith(module) for name in want), module
    assert sorted(got["python_exits"]) == sorted(want)
    assert not _differences(got["python_exits"], want)


def test_layout_header_on_its_own(tmp_path):
    compiler = shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    assert os.path.exists(compiler), "no clang++ found for the stand-alone layout check"
    exe = str(tmp_path / "lexical_proj_layout_check")
    cmd = [compiler, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(HERE, "lexical_proj_layout_check.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert run.stdout.startswith("lexical proj layout ok:"), run.stdout
    assert int(run.stdout.split(":")[1].split()[0]) > 700 * 60, run.stdout          # more than 700 shapes of the grid, over 60 checks each


# ---- what the heads compute
@pytest.fixture(scope="module")
def pinned_gpu(gen):
    with open(gen.PATH_GPU) as f:
        return json.load(f)


def _module_equals_the_parent(gen, pinned_gpu, name, collect):
    import torch
    mod = importlib.import_module("dhr_amd." + name)
    want, got = gen.leaves(pinned_gpu[name]), gen.leaves(collect(torch, mod))
    assert sorted(got) == sorted(want)
    assert not _differences(got, want)
    return want


@pytest.mark.gpu
def test_lexical_equals_the_parent(gen, pinned_gpu):
    want = _module_equals_the_parent(gen, pinned_gpu, "lexical", gen.collect_lexical)
    assert len(want) >= 9 * 25                                     # nine inputs (device, offset views, numpy) x every record mode
    for a, b in (("device_float16", "device_float32"), ("device_float16", "device_float16_offset4"), ("device_float16", "device_float16_packed"),
                 ("numpy_float16", "numpy_float32")):
        assert pinned_gpu["lexical"][a] == pinned_gpu["lexical"][b], (a, b)      # the same values, whatever dtype or alignment brings them


@pytest.mark.gpu
def test_lexical_proj_equals_the_parent(gen, pinned_gpu):
    _module_equals_the_parent(gen, pinned_gpu, "lexical_proj", gen.collect_lexical_proj)
    p = pinned_gpu["lexical_proj"]
    for dt in ("float16", "bfloat16"):
        assert p[dt + "_bias_float32"] == p[dt + "_offset4"] == p[dt + "_weight_row_stride"], dt
        assert p[dt + "_bias_float32"] != p[dt + "_bias_none"], dt


@pytest.mark.gpu
def test_lexical_train_equals_the_parent(gen, pinned_gpu):
    _module_equals_the_parent(gen, pinned_gpu, "lexical_train", gen.collect_lexical_train)
    p = pinned_gpu["lexical_train"]
    for dt in ("float16", "bfloat16", "float32"):                  # the docstring's promise: the view and the whole tensor give the same bits
        assert p[dt + "_whole_skip1"]["reps"] == p[dt + "_view_skip0"]["reps"] and p[dt + "_whole_skip1"]["tok"] == p[dt + "_view_skip0"]["tok"]


@pytest.mark.gpu
def test_lexical_proj_train_equals_the_parent(gen, pinned_gpu):
    _module_equals_the_parent(gen, pinned_gpu, "lexical_proj_train", gen.collect_lexical_proj_train)
    p = pinned_gpu["lexical_proj_train"]
    for dt in ("float16", "bfloat16"):
        assert p[dt + "_whole_skip1"]["reps"] == p[dt + "_view_skip0"]["reps"] == p[dt + "_frozen_projector"]["reps"]
        assert "grad_weight_after_sum" not in p[dt + "_frozen_projector"] and "grad_hidden_after_sum" not in p[dt + "_detached_hidden"]
        for hb in (776, 1024):                                      # the slab cut of the gradient passes, and the split's partial sums
            assert len(p["shape_b_h%d_%s" % (hb, dt)]) == 10


@pytest.mark.gpu
def test_second_block_of_the_staged_loop(gen, pinned_gpu):
    """fp32 numpy logits [18, 128, 30522]: 17 rows fill the staging block of dhr_lexical_head, the 18th runs as a second block.  Bit for bit the
    reps of the same call on device memory, and the parent's."""
    import torch
    from dhr_amd import lexical as LX
    host, dev = gen.staged_second_block(torch, LX)
    assert host == dev
    assert {"host": host, "device": dev} == pinned_gpu["staged_second_block"]
