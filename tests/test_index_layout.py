"""The host side of the index build on the CPU.  (i) dhr_amd/csrc/index_layout.h -- the layout plan, the column-step rule of the two int8 images, the
bucket deal: tests/index_layout_check.cpp includes that header alone and asserts its invariants over a grid of descriptors and a table of
hand-derived layouts, built as host C++ with AddressSanitizer and UBSan and run as a plain executable.  (ii) The descriptor rules of
dhr_index_create, which sit in front of its first device call: every rule with its status and message, and descriptors that break two rules
at once, which must report the one that comes first."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "dhr_amd", "csrc")
sys.path.insert(0, ROOT)

from dhr_amd import _lib  # noqa: E402


def _compiler():
    path = shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    assert os.path.exists(path), "no clang++ found for the stand-alone layout check"
    return path


def test_index_layout_invariants(tmp_path):
    exe = str(tmp_path / "index_layout_check")
    cmd = [_compiler(), "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(HERE, "index_layout_check.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert run.stdout.startswith("index layout ok:"), run.stdout
    assert int(run.stdout.split(":")[1].split()[0]) > 1_000_000, run.stdout
    print(run.stdout.strip())


# ---- the descriptor rules (no device is touched: every descriptor here is refused before hipSetDevice)
VALUE = np.zeros((8, 32), np.float16)
INDEX = np.zeros((8, 16), np.uint8)
NO_VALUE = {"value": None}
BASE = dict(device=0, mem_kind=_lib.MEM_HOST, n_rows=8, d_dlr=16, d_cls=16, value=VALUE.ctypes.data, ld_value=32, index=INDEX.ctypes.data,
            index_dtype=_lib.IDX_U8, idx_buckets=0, ld_index=16, row_offset=0)
DENSE_ONLY = dict(d_dlr=0, index=None, index_dtype=_lib.IDX_NONE, ld_index=0)
WIDE = dict(d_dlr=8185, d_cls=4, ld_value=8189, ld_index=8185)      # 8189 columns: 8196 with the seven zero slices the library appends
MSG_VALUE, MSG_LD_INDEX, MSG_ROWS, MSG_WIDTHS = "bad value pointer / ld_value", "bad ld_index", "n_rows must be in [1, 2^32-256)", "bad d_dlr/d_cls"
MSG_IFF = "an index array is required iff d_dlr > 0 (dense-only: index=NULL, d_dlr=0)"
MSG_DTYPE, MSG_WIDE, MSG_MEM = "bad index_dtype", "more than 8192 columns", "bad mem_kind"
MSG_BUCKETS = "idx_buckets must be 0 (default: 2), 1 (ungated bound) or 2: the bucket-split operands of more than two buckets went with the K-step tile layout (round 6)"
INVALID, UNSUPPORTED = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED

RULES = {
    "ld_value_short": (dict(ld_value=31), INVALID, MSG_VALUE),
    "ld_value_short_of_the_callers_width": (dict(d_dlr=12, ld_value=27, ld_index=12), INVALID, MSG_VALUE),
    "no_value_pointer": (NO_VALUE, INVALID, MSG_VALUE),
    "ld_index_short": (dict(ld_index=15), INVALID, MSG_LD_INDEX),
    "no_rows": (dict(n_rows=0), INVALID, MSG_ROWS),
    "too_many_rows": (dict(n_rows=0xFFFFFF00), INVALID, MSG_ROWS),
    "negative_width": (dict(d_cls=-1), INVALID, MSG_WIDTHS),
    "no_columns": (dict(DENSE_ONLY, d_cls=0), INVALID, MSG_WIDTHS),
    "gated_columns_without_an_index": (dict(index=None), INVALID, MSG_IFF),
    "gated_columns_with_dtype_none": (dict(index_dtype=_lib.IDX_NONE), INVALID, MSG_IFF),
    "an_index_without_gated_columns": (dict(d_dlr=0), INVALID, MSG_IFF),
    "index_dtype_above": (dict(index_dtype=_lib.IDX_I16 + 1), INVALID, MSG_DTYPE),
    "index_dtype_below": (dict(index_dtype=-1), INVALID, MSG_DTYPE),
    "too_wide_once_padded": (WIDE, UNSUPPORTED, MSG_WIDE),
    "too_wide_dense_only": (dict(DENSE_ONLY, d_cls=8193, ld_value=8193), UNSUPPORTED, MSG_WIDE),
    "negative_idx_buckets": (dict(idx_buckets=-1), INVALID, MSG_BUCKETS),
    "three_idx_buckets": (dict(idx_buckets=3), UNSUPPORTED, MSG_BUCKETS),
    "mem_kind": (dict(mem_kind=7), INVALID, MSG_MEM),
    # two rules at once: the first one in the order of the checks is reported
    "ld_value_before_n_rows": (dict(ld_value=31, n_rows=0), INVALID, MSG_VALUE),
    "ld_index_before_mem_kind": (dict(ld_index=15, mem_kind=7), INVALID, MSG_LD_INDEX),
    "ld_index_before_index_dtype": (dict(ld_index=15, index_dtype=_lib.IDX_I16 + 1), INVALID, MSG_LD_INDEX),
    "n_rows_before_value_pointer": (dict(NO_VALUE, n_rows=0), INVALID, MSG_ROWS),
    "widths_before_value_pointer": (dict(NO_VALUE, d_cls=-1), INVALID, MSG_WIDTHS),
    "value_pointer_before_index_dtype": (dict(NO_VALUE, index_dtype=_lib.IDX_I16 + 1), INVALID, MSG_VALUE),
    "index_dtype_before_width": (dict(WIDE, index_dtype=_lib.IDX_I16 + 1), INVALID, MSG_DTYPE),
    "width_before_idx_buckets": (dict(WIDE, idx_buckets=3), UNSUPPORTED, MSG_WIDE),
    "idx_buckets_before_mem_kind": (dict(idx_buckets=3, mem_kind=7), UNSUPPORTED, MSG_BUCKETS),
}


@pytest.mark.parametrize("rule", sorted(RULES))
def test_descriptor_rules_without_a_device(rule):
    change, status, message = RULES[rule]
    lib = _lib.load()
    desc = _lib.IndexDesc(**dict(BASE, **change))
    h = C.c_void_p(1)
    assert lib.dhr_index_create(C.byref(desc), C.byref(h)) == status
    assert lib.dhr_last_error().decode() == message
    # (the two leading-dimension rules are checked before the output handle is cleared, as ever)
    untouched = message == MSG_LD_INDEX or (message == MSG_VALUE and "value" not in change)
    assert h.value == (1 if untouched else None)


def test_null_arguments_without_a_device():
    lib = _lib.load()
    desc = _lib.IndexDesc(**BASE)
    h = C.c_void_p()
    for args in ((None, C.byref(h)), (C.byref(desc), None)):
        assert lib.dhr_index_create(*args) == INVALID
        assert lib.dhr_last_error().decode() == "null argument"
