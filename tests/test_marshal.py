"""CPU-only tests of dhr_amd._marshal, the layer between tensors and the C ABI: when a strided view is read in place, which strides are
reported, and the whole argument tuple the host-array paths of the ops hand to the library (recorded, no library is loaded)."""
import ctypes as C

import numpy as np
import pytest

from dhr_amd import _lib
from dhr_amd import _marshal as M

N = 64                                   # elements of the base buffer every view is cut from


def _np_view(shape, strides, offset=0):
    base = np.arange(N, dtype=np.float32)
    v = np.lib.stride_tricks.as_strided(base[offset:], shape, tuple(4 * s for s in strides))
    return base, v


def _torch_view(shape, strides, offset=0):
    import torch
    base = torch.arange(N, dtype=torch.float32)
    return base, base.as_strided(shape, strides, offset)


# (shape, strides in elements, offset, disjoint, read in place?, reported outer strides, the parent helper this decision is taken from)
CASES = [
    ((3, 5), (5, 1), 0, True, True, (5,), "every helper: packed"),
    ((3, 5), (8, 1), 2, True, True, (8,), "gip_scores._rows2d: rows of a wider record"),
    ((3, 5), (4, 1), 0, True, False, (5,), "gip_scores._rows2d: overlapping rows are copied"),
    ((3, 5), (0, 1), 0, True, False, (5,), "train_loss._matrix: an expanded row is copied"),
    ((3, 5), (1, 3), 0, True, False, (5,), "every helper: a transposed view is copied"),
    ((1, 5), (1, 1), 3, True, True, (5,), "train_loss._matrix + _arg: one row, stride normalised"),
    ((1, 5), (7, 1), 3, True, True, (5,), "train_loss._matrix + _arg: one row, stride normalised"),
    ((1, 5), (0, 1), 3, True, True, (5,), "aggretriever_train._rows + _ld: one row, stride normalised"),
    ((3, 1), (2, 1), 1, True, True, (2,), "train_loss._matrix: one column"),
    ((3, 1), (2, 4), 1, True, True, (2,), "train_loss._matrix: the stride of one column is free"),
    ((0, 5), (5, 1), 0, True, True, (5,), "train_loss._matrix: empty, as it is"),
    ((3, 0), (5, 1), 0, True, True, (5,), "aggretriever_train._rows: empty, as it is"),
    ((2, 3, 4), (12, 4, 1), 0, True, True, (12, 4), "every helper: packed"),
    ((2, 3, 4), (16, 4, 1), 4, True, True, (16, 4), "lexical_train._strided: base[:, 1:] of [2, 4, 4]"),
    ((2, 3, 4), (4, 4, 1), 0, False, True, (4, 4), "maxsim_scores._tokens3d: batch stride >= D, batches overlap"),
    ((2, 3, 4), (4, 4, 1), 0, True, False, (12, 4), "lexical_train._strided: batch stride < (L - 1) * st + V is copied"),
    ((1, 3, 4), (13, 5, 1), 1, False, True, (15, 5), "maxsim_scores._ptr_lds: one batch, reported L * st"),
    ((2, 1, 4), (7, 3, 1), 1, False, True, (7, 4), "maxsim_scores._ptr_lds: one token, reported D"),
    ((2, 3, 4), (24, 8, 2), 0, True, False, (12, 4), "every helper: a strided last dimension is copied"),
]


@pytest.mark.parametrize("make", [_np_view, _torch_view], ids=["numpy", "torch"])
@pytest.mark.parametrize("shape,strides,offset,disjoint,in_place,lds,role", CASES, ids=[f"{c[0]}-{c[1]}-{'disjoint' if c[3] else 'D'}" for c in CASES])
def test_in_place_or_copy_and_the_reported_strides(make, shape, strides, offset, disjoint, in_place, lds, role):
    base, v = make(shape, strides, offset)
    out, ld = M.as_read(v, disjoint=disjoint)
    assert ld == lds, role
    assert tuple(out.shape) == shape
    if in_place:
        assert out is v, role
        if 0 not in shape:                                               # (torch reports a null pointer for an empty tensor)
            assert M.data_ptr(out) == M.data_ptr(base) + 4 * offset, role
    else:
        packed = tuple(int(np.prod(shape[i + 1:])) for i in range(len(shape)))
        assert out is not v and M.strides(out) == packed, role
        assert not M.data_ptr(base) <= M.data_ptr(out) < M.data_ptr(base) + 4 * N, role
        assert np.array_equal(np.asarray(out), np.asarray(v))
    assert M.lds(out) == ld


def test_numpy_byte_strides():
    """gip_scores._rows2d / lexical._inputs on numpy: a byte stride that is no multiple of the item size, or a negative one, is copied"""
    rec = np.zeros((3, 5), dtype=np.dtype([("a", "<f4"), ("b", "u1")]))
    rec["a"] = np.arange(15, dtype=np.float32).reshape(3, 5)
    field = rec["a"]
    assert field.strides == (25, 5) and field.itemsize == 4
    out, ld = M.as_read(field)
    assert out is not field and out.strides == (20, 4) and ld == (5,) and np.array_equal(out, field)
    a = np.arange(15, dtype=np.float32).reshape(3, 5)
    out, ld = M.as_read(a[::-1])
    assert out.strides == (20, 4) and ld == (5,) and np.array_equal(out, a[::-1]) and not np.shares_memory(out, a)
    one = a[::-1][:1]                                                    # one row: its (negative) stride is free
    out, ld = M.as_read(one)
    assert out is one and ld == (5,)


def test_host_operands_get_the_null_stream_device_0_and_host_memory():
    import torch
    for a in (np.zeros((2, 3), np.float32), torch.zeros((2, 3))):
        assert M.stream(a) is None and M.device(a) == 0 and M.mem_kind(a) == _lib.MEM_HOST
    assert M.data_ptr(None) is None


def test_dtype_choices_and_outputs():
    import torch
    f16, f32, f64 = (np.zeros((1, 1), t) for t in (np.float16, np.float32, np.float64))
    assert M.common_dtype(f16, f16, M.FLOATS, "float32") == "float16" and M.common_dtype(f32, f32, M.FLOATS, "float32") == "float32"
    assert M.common_dtype(f16, f32, M.FLOATS, "float32") == "float32" and M.common_dtype(f64, f64, M.FLOATS, "float32") == "float32"
    i8, i64 = torch.zeros((1, 1), dtype=torch.int8), torch.zeros((1, 1), dtype=torch.int64)
    assert M.common_dtype(i8, i8, M.NARROW, "int16") == "int8" and M.common_dtype(i8, i64, M.NARROW, "int16") == "int16"
    assert M.values(f16) is f16 and M.values(f64).dtype == np.float32 and M.values(i64).dtype == torch.float32
    assert M.cast(i8, torch.int8) is i8 and M.cast(i8, "int16").dtype == torch.int16 and M.cast(f32, f32.dtype) is f32
    out = M.empty(f16, (2, 3), "int16")
    assert isinstance(out, np.ndarray) and out.shape == (2, 3) and out.dtype == np.int16
    out = M.empty(i8, (2, 3), torch.float16)
    assert isinstance(out, torch.Tensor) and tuple(out.shape) == (2, 3) and out.dtype == torch.float16 and out.device == i8.device


def test_grad_rows():
    import torch
    g = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    out, ld = M.grad_rows(g, 3, 4)
    assert out.data_ptr() == g.data_ptr() and tuple(out.stride()) == (4, 1) and ld == 4 and out.dtype == torch.float32      # the tensor itself
    out, ld = M.grad_rows(g.t(), 4, 3)
    assert out.data_ptr() != g.data_ptr() and tuple(out.stride()) == (3, 1) and ld == 3 and torch.equal(out, g.t())
    x = torch.zeros((3, 4), requires_grad=True)
    seen = []
    x.register_hook(seen.append)
    x.sum().backward()                                                   # the gradient of sum() is an expanded scalar: strides (0, 0)
    assert tuple(seen[0].stride()) == (0, 0)
    out, ld = M.grad_rows(seen[0], 3, 4)
    assert tuple(out.stride()) == (4, 1) and ld == 4 and torch.equal(out, torch.ones((3, 4)))
    out, ld = M.grad_rows(g.double(), 3, 4, torch.float16)
    assert out.dtype == torch.float16 and ld == 4 and not out.requires_grad


class _Recorder:
    """stands in for the loaded library: every dhr_* call is recorded and answers DHR_OK, a *_workspace call a byte count"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 256 if name.endswith("_workspace") else _lib.DHR_OK
        return call


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    return rec


def test_gip_scores_host_call(recorder):
    """n_q = 3, n_p = 4, dims = 8, fp32 values and uint8 groups cut from 12-column bases: read in place with row stride 12"""
    from dhr_amd import gip_scores as GS
    bq, bp = np.zeros((3, 12), np.float32), np.zeros((4, 12), np.float32)
    bqi, bpi = np.zeros((3, 12), np.uint8), np.zeros((4, 12), np.uint8)
    out = GS.gip_scores(bq[:, 2:10], bqi[:, 1:9], bp[:, 4:], bpi[:, :8])
    assert out.shape == (3, 4) and out.dtype == np.float32
    assert recorder.calls == [("dhr_gip_scores", (0, _lib.MEM_HOST, bq.ctypes.data + 8, 12, bqi.ctypes.data + 1, 12, 3, bp.ctypes.data + 16, 12,
                                                  bpi.ctypes.data, 12, 4, 8, _lib.VAL_F32, _lib.IDX_U8, 0, out.ctypes.data, 4, None, 0, None))]


def test_maxsim_scores_host_call(recorder):
    """A = 2, B = 3, Lq = 2, Lp = 3, D = 5 as base[:, 1:, :5] of bases with D padded to 8: token stride 8, batch stride (L + 1) * 8"""
    from dhr_amd import maxsim_scores as MS
    bq, bp = np.zeros((2, 3, 8), np.float32), np.zeros((3, 4, 8), np.float32)
    out = MS.maxsim_scores(bq[:, 1:, :5], bp[:, 1:, :5])
    assert out.shape == (2, 3) and out.dtype == np.float32
    assert recorder.calls == [("dhr_maxsim_scores", (0, _lib.MEM_HOST, bq.ctypes.data + 32, 8, 24, 2, 2, bp.ctypes.data + 32, 8, 32, 3, 3, 5, _lib.VAL_F32,
                                                     0, out.ctypes.data, 3, None, None))]


def test_train_loss_host_call(recorder):
    """R = 3, C = 5 CPU tensors cut from 8-column bases, no teacher, nothing to differentiate: host memory, no workspace, null gradients"""
    import torch
    from dhr_amd import train_loss as TL
    bl, bs = torch.zeros((3, 8)), torch.zeros((3, 8), dtype=torch.float16)
    loss, scores = TL.hybrid_loss(bl[:, 1:6], bs[:, 3:], train_n_passages=2, lamb=0.5, weights=(1.0, 0.5, 0.25))
    (name, a), = recorder.calls
    assert name == "dhr_train_loss"
    assert a[:16] == (0, _lib.MEM_HOST, bl.data_ptr() + 4, _lib.VAL_F32, 8, bs.data_ptr() + 6, _lib.VAL_F16, 8, None, _lib.VAL_F32, 0, 3, 5, 2, 0.5, 1.0)
    assert list(a[16]) == [1.0, 0.5, 0.25] and list(a[17]) == [1.0, 0.75, 0.25] and isinstance(a[16], C.c_float * 3)
    assert a[18:] == (loss.data_ptr(), scores.data_ptr(), 5, None, 5, None, 5, None, 0, None)


def test_lexical_head_host_call(recorder):
    """B = 2, T = 3, V = 32 fp16 logits as base[:, 1:, :32] of a [2, 4, 40] base: batch stride 160, token stride 40; weights and mask are
    packed fp32 copies"""
    from dhr_amd import lexical as LX
    base = np.zeros((2, 4, 40), np.float16)
    out = LX.lexical_reps(base[:, 1:, :32], np.ones((2, 3, 1), np.float16), np.ones((2, 3), np.int64))
    (name, a), = recorder.calls
    assert name == "dhr_lexical_head" and out.shape == (2, 32) and out.dtype == np.float32
    assert a[:10] == (0, _lib.MEM_HOST, _lib.LEX_RAW, base.ctypes.data + 80, _lib.VAL_F16, 2, 3, 32, 160, 40)
    assert isinstance(a[10], int) and a[10] and isinstance(a[12], int) and a[12] and a[10] != a[12]
    assert (a[11], a[13]) + a[14:] == (3, 3, 0, 0, out.ctypes.data, _lib.VAL_F32, 32, None, _lib.IDX_NONE, 0, None, _lib.VAL_F16, 0, 0, None, None)


def test_densify_host_call(recorder):
    """densify_into on [2, 34] reps cut from a 40-column base (remove 2, dims 8), into the first columns of 12-wide records"""
    from dhr_amd.densify import densify_into
    base, val, idx = np.zeros((2, 40), np.float32), np.zeros((2, 12), np.float16), np.zeros((2, 9), np.uint8)
    densify_into(base[:, 3:37], val, idx, dims=8, remove_dims=2)
    assert recorder.calls == [("dhr_densify", (0, _lib.MEM_HOST, base.ctypes.data + 12, _lib.VAL_F32, 40, 2, 34, 2, 8, val.ctypes.data, _lib.VAL_F16, 12,
                                               idx.ctypes.data, _lib.IDX_U8, 9, None))]
