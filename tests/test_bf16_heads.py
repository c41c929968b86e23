"""bfloat16 in the four lexical heads: dhr_amd.lexical, lexical_train, lexical_proj and lexical_proj_train on DHR_VAL_BF16 (include/dhr_hip.h).

What is checked against what:
 - a bf16 value widens to fp32 exactly and the kernels keep every fp32 operation in its place, so wherever bf16 and fp16 tensors hold the same
   values (the goldens: the CPU part asserts that every input array of the four fixtures is a bf16 value) the forward outputs must be the SAME
   BITS as those of the fp16 call, and so must every fp32 output of the backward that never sees a 16-bit rounding (dL/dw of lexical_train);
 - gradients that are rounded to bf16, or that pass through the bf16 rounding of the logit gradient in front of the two gradient GEMMs, are held
   to the bounds of tests/test_lexical_train.py (kappa, b_dx, b_dw) and tests/test_lexical_proj_train.py (the (H + 2) A widening, n u sum
   |terms|) with the two fp16 constants replaced: one rounding to bf16 is at most 2^-8 |truth| (UB16; 8 significant bits, round to nearest
   even), and below the normal range a flush is allowed, 2^-126 (SUBB16).  truth64 below is test_lexical_proj_train.truth64 with those two as
   parameters; nothing else of the bounds changes and no tolerance is picked by hand.  Where truth and bound are zero the result is exactly zero;
 - range: bf16 keeps fp32's exponent, so hidden * 2^40 against weight * 2^-40 is the same product exactly (an fp16 detour would overflow and
   underflow), and a logit row of +-2^100 is an ordinary row.

Random data is drawn with numpy on the CPU from fixed seeds and rounded to bf16 there.  Measured worst error / bound on an MI355X:
profiles/bf16_heads.txt (every GPU test prints its own).

CPU part (-m "not gpu"): constants, statuses of the six entry points, the wrappers' errors, the fixtures are bf16 values, the near-tie cap of
the seeds.  GPU part: -m gpu."""
import os
import re

import numpy as np
import pytest

from dhr_amd import _lib
from tests.test_lexical_head import _head
from tests.test_lexical_proj import _call
from tests.test_lexical_proj_train import RANDOM, _bwd, _train, random_case
from tests.test_lexical_train import ATOL, RTOL, U32, _bwd_args, _train_args, backward64, check_routing, forward64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = {k: os.path.join(ROOT, "tests", "golden", k + "_golden.npz") for k in ("lexical", "lexical_train", "lexical_proj", "lexical_proj_train")}
UB16, SUBB16 = 2.0 ** -8, 2.0 ** -126
U16, SUB16 = 2.0 ** -11, 2.0 ** -25                      # (fp16, where a gradient comes back in fp16)
LOGITS = [(5, 70, 762, 11), (3, 150, 1030, 12), (33, 40, 515, 13), (2, 9, 202, 14),          # B, T, V, seed
          (512, 2, 8, 15), (512, 2, 9, 15)]       # 512 workgroups of 16 tokens in the backward's reduction pass; 16- and 18-byte bf16 rows
BF16 = _lib.VAL_BF16 if hasattr(_lib, "VAL_BF16") else 2


def rb(a):
    """float values rounded to bf16 (nearest even), as float32"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def logits_case(B, T, V, seed):
    """-> the model's logits [B, T + 1, V] (bf16 values in float32; tokens 1 .. T are the recipe of the issue), w [B, T] fp32 of mixed signs,
    mask [B, T] (ragged, a masked token between live ones, the last passage fully masked where B > 2), G [B, V] fp32 (a tenth zeros)"""
    rng = np.random.default_rng(seed)
    x = rb(rng.standard_normal((B, T, V)) * 3)
    first = rb(rng.standard_normal((B, 1, V)) * 3)
    w = rng.standard_normal((B, T)).astype(np.float32)
    lens = rng.integers(1, T + 1, B)
    lens[0] = T
    mask = (np.arange(T)[None] < lens[:, None]).astype(np.int64)
    mask[1, min(2, T - 1)] = 0
    if B > 2:
        mask[-1] = 0
    G = (rng.standard_normal((B, V)) * (rng.random((B, V)) > 0.1)).astype(np.float32)
    return np.concatenate([first, x], 1), w, mask, G


def random_case_bf16(B, T, V, H, seed):
    """random_case of tests/test_lexical_proj_train.py, the same draws in the same order, rounded to bf16 instead of fp16 (float32 arrays)"""
    rng = np.random.default_rng(seed)
    hidden = rb(rng.standard_normal((B, T + 1, H)))
    W = rb(rng.standard_normal((V, H)) * (2 / np.sqrt(H)))
    rest = random_case(B, T, V, H, seed)[2:]                                       # bias, w, mask, G: not rounded there either
    return (hidden, W) + tuple(rest)


def truth64(hidden, W, bias, w, m, G, tok=None, inexact=False, u16=UB16, sub16=SUBB16, what=""):
    """tests/test_lexical_proj_train.py's truth64 with the rounding unit of the logit gradient as a parameter (u16 = 0: it is not rounded).
    hidden [B, T, H], W [V, H], bias [V] or None: the VALUES the kernels read.  -> truths dh, dW, db, dw, reps, a; bounds b_dh, b_dW, b_db, b_dw;
    ties (counted through check_routing where tok is given) and near"""
    hidden, W, w, m, G = (np.asarray(a).astype(np.float64) for a in (hidden, W, w, m, G))
    bias = np.zeros(W.shape[0]) if bias is None else np.asarray(bias).astype(np.float64)
    B, T, H = hidden.shape
    V = W.shape[0]
    aW = np.abs(W)
    M = max(1, int((m != 0).sum()))
    r = dict(dh=np.zeros((B, T, H)), b_dh=np.zeros((B, T, H)), dW=np.zeros((V, H)), db=np.zeros(V), dw=np.zeros((B, T)), b_dw=np.zeros((B, T)),
             reps=np.zeros((B, V)), a=np.zeros((B, V), np.int64), ties=0, near=0)
    e_dW, s_dW, e_db, s_db = np.zeros((V, H)), np.zeros((V, H)), np.zeros(V), np.zeros(V)
    for b in range(B):
        x = (hidden[b] @ W.T + bias)[None]
        w1, m1, G1 = w[b:b + 1], m[b:b + 1], G[b:b + 1]
        p, d, reps, a, near, c = forward64(x, w1, m1)
        t1 = a if tok is None else np.asarray(tok[b:b + 1]).astype(np.int64)
        r["near"] += int(near.sum())
        if tok is not None:
            r["ties"] += check_routing(t1, a, near, c, f"{what} passage {b}")
        dx, b_dx, dw, b_dw = backward64(p, d, w1, m1, G1, t1)
        if inexact:
            A = (np.abs(hidden[b]) @ aW.T + np.abs(bias)).max(-1)[None]                          # [1, T]
            delta = 2 * (H + 2) * A
            route = t1[:, None, :] == np.arange(T)[None, :, None]
            gp = route * G1[:, None, :] * p
            S1g = np.abs(gp).sum(-1)
            R = route * G1[:, None, :] * (w1 * m1)[..., None]
            b_dx = b_dx + 2 * delta[..., None] * U32 * p * (np.abs(R) + (np.abs(w1 * m1) * S1g)[..., None])
            b_dw = b_dw + delta * U32 * np.abs(m1) * S1g
        dx, b_dx = dx[0], b_dx[0]
        live = (dx != 0) | (b_dx != 0)
        e = np.where(live, b_dx + np.maximum(u16 * np.abs(dx), sub16), 0.0) if u16 else b_dx
        hb = hidden[b]
        r["dh"][b], r["b_dh"][b] = dx @ W, e @ aW + V * U32 * ((np.abs(dx) + e) @ aW)
        r["dW"] += dx.T @ hb
        e_dW += e.T @ np.abs(hb)
        s_dW += (np.abs(dx) + e).T @ np.abs(hb)
        r["db"] += dx.sum(0)
        e_db += b_dx.sum(0)
        s_db += np.abs(dx).sum(0)
        r["dw"][b], r["b_dw"][b], r["reps"][b], r["a"][b] = dw[0], b_dw[0], reps[0], a[0]
    r["b_dW"] = e_dW + M * U32 * s_dW
    r["b_db"] = e_db + M * U32 * s_db
    return r


WORST = {}


def within(got, truth, bound, what, out=None):
    """|got - truth| <= bound + the one rounding of an output of dtype `out` ("bf16", "fp16" or None: fp32); exactly zero where both are
    zero.  -> worst error / bound, also kept in WORST under the text after the last ':' of `what`"""
    got = np.asarray(got).astype(np.float64)
    assert got.shape == truth.shape, (what, got.shape, truth.shape)
    u, sub = {"bf16": (UB16, SUBB16), "fp16": (U16, SUB16), None: (0.0, 0.0)}[out]
    tol = bound + (np.where(truth != 0, np.maximum(u * np.abs(truth), sub), 0.0) if out else 0.0)
    err = np.abs(got - truth)
    bad = ~(err <= tol)
    worst = float((err / np.where(tol > 0, tol, 1.0))[tol > 0].max()) if (tol > 0).any() else 0.0
    key = what.split(":")[-1].strip() + (" (" + out + " out)" if out else " (fp32 out)")
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print(f"{what}: max error / bound = {worst:.4f}; entries with a zero bound that are not zero: {int((err[tol == 0] != 0).sum())}")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} entries outside the bound (worst error / bound {worst:.3f})"
    return worst


# ------------------------------------------------------------------------------------------ CPU part
def test_abi_constants():
    assert _lib.VAL_BF16 == 2 and (_lib.VAL_F16, _lib.VAL_F32) == (0, 1)
    header = open(os.path.join(ROOT, "include", "dhr_hip.h")).read()
    assert re.search(r"enum dhr_val_dtype \{[^}]*DHR_VAL_BF16 = 2[^}]*\}", header)
    assert _lib.load().dhr_version() == 105
    import torch
    assert _lib._val_code(torch.zeros(1, dtype=torch.bfloat16), bf16=True) == 2
    with pytest.raises(_lib.DhrError):                                             # every other argument keeps refusing it in Python
        _lib._val_code(torch.zeros(1, dtype=torch.bfloat16))


def _device_args():
    """real device memory for the valid calls where there is a device: B = 2, T = 3 after one skipped token, V = 32, H = 16"""
    import torch
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")            # noqa: E731
    bf, f32 = torch.bfloat16, torch.float32
    t = dict(lg=z((2, 4, 32), bf), hid=z((2, 4, 16), bf), W=z((32, 16), bf), bias=z((32,), bf), w=torch.ones((2, 3), device="cuda"),
             m=torch.ones((2, 3), device="cuda"), reps=z((2, 32), f32), tok=z((2, 32), torch.int16), pwin=z((2, 32), f32), g=torch.ones((2, 32), device="cuda"),
             dx=z((2, 4, 32), bf), dw=z((2, 3), f32), gh=z((2, 4, 16), bf), gw=z((32, 16), bf), gb=z((32,), bf), val=z((2, 8), torch.float16),
             idx=z((2, 8), torch.uint8), ws=z((1 << 20,), torch.uint8))
    return t, {k: v.data_ptr() for k, v in t.items()}


def test_statuses_of_the_six_entry_points():
    import torch
    lib = _lib.load()
    OK, INVALID = _lib.DHR_OK, _lib.ERR_INVALID
    lg = np.zeros((2, 3, 32), np.uint16)                                           # bf16 bits in host memory
    w, m = np.ones((2, 3), np.float32), np.ones((2, 3), np.float32)
    val, idx = np.zeros((2, 8), np.float16), np.zeros((2, 8), np.uint8)
    host = dict(logits=lg.ctypes.data, w=w.ctypes.data, m=m.ctypes.data, val=val.ctypes.data, idx=idx.ctypes.data)
    calls = {
        "dhr_lexical_head": lambda **kw: _head(lib, **{**host, **kw}),
        "dhr_lexical_head_train": lambda **kw: lib.dhr_lexical_head_train(*_train_args(**{("dtype" if k == "value_dtype" else k): v for k, v in kw.items()})),
        "dhr_lexical_head_backward": lambda **kw: lib.dhr_lexical_head_backward(*_bwd_args(**{("dtype" if k == "value_dtype" else k): v for k, v in kw.items()})),
        "dhr_lexical_proj_head": lambda **kw: _call(lib, **kw),
        "dhr_lexical_proj_train": lambda **kw: _train(lib, **kw),
        "dhr_lexical_proj_backward": lambda **kw: _bwd(lib, **kw),
    }
    for name, call in calls.items():
        assert call(value_dtype=BF16, batch=0) == OK, name
        for bad in (3, 5, -1):
            assert call(value_dtype=bad) == INVALID and call(value_dtype=bad, batch=0) == INVALID, (name, bad)
    for name in ("dhr_lexical_proj_head", "dhr_lexical_proj_train", "dhr_lexical_proj_backward"):
        assert calls[name](value_dtype=BF16, bias_dtype=BF16, batch=0) == OK, name
        assert calls[name](value_dtype=BF16, bias_dtype=_lib.VAL_F32, batch=0) == OK, name
        assert calls[name](value_dtype=BF16, bias_dtype=_lib.VAL_F16, batch=0) == OK, name       # the bf16 kernels read any of the three
        assert calls[name](value_dtype=_lib.VAL_F16, bias_dtype=BF16, batch=0) == _lib.ERR_UNSUPPORTED, name   # the fp16 kernels: fp32 or fp16
        for bad in (3, 5, -1):
            assert calls[name](value_dtype=BF16, bias_dtype=bad, batch=0) == INVALID, (name, bad)
        assert calls[name](value_dtype=_lib.VAL_F32) == _lib.ERR_UNSUPPORTED, name                # fp32 operands stay unbuilt
    # the records the encode heads write, and the [CLS] reps they copy, are never bf16
    assert calls["dhr_lexical_head"](value_dtype=BF16, val_dtype=BF16, batch=0) == INVALID
    assert calls["dhr_lexical_proj_head"](value_dtype=BF16, val_dtype=BF16, batch=0) == INVALID
    assert calls["dhr_lexical_head"](value_dtype=BF16, cls=val.ctypes.data, cls_dtype=BF16, cls_dim=2, ld_cls=2, ld_val=10, batch=0) == INVALID
    # the gradients of the projection backward: each of the three dtypes on its own
    assert calls["dhr_lexical_proj_backward"](value_dtype=BF16, gh_dtype=BF16, gw_dtype=BF16, gb_dtype=BF16, batch=0) == OK
    assert calls["dhr_lexical_proj_backward"](value_dtype=BF16, gh_dtype=BF16, gw_dtype=_lib.VAL_F32, gb_dtype=_lib.VAL_F16, batch=0) == OK
    for k in ("gh_dtype", "gw_dtype", "gb_dtype"):                                             # ... but a bf16 gradient needs bf16 operands
        assert calls["dhr_lexical_proj_backward"](value_dtype=_lib.VAL_F16, batch=0, **{k: BF16}) == _lib.ERR_UNSUPPORTED, k
        assert calls["dhr_lexical_proj_backward"](value_dtype=BF16, batch=0, **{k: 3}) == INVALID, k
    assert calls["dhr_lexical_head_backward"](value_dtype=BF16, batch=0) == OK                    # (its gradient has the logits' dtype)
    # the shared predicate was not widened: the standalone aggregate still refuses code 2 on either side
    reps, out = np.zeros((2, 32), np.float32), np.zeros((2, 8), np.float32)
    assert lib.dhr_aggregate(0, _lib.MEM_HOST, reps.ctypes.data, BF16, 32, 2, 32, 8, 0, 1, out.ctypes.data, _lib.VAL_F32, 8, None) == INVALID
    assert lib.dhr_aggregate(0, _lib.MEM_HOST, reps.ctypes.data, _lib.VAL_F32, 32, 2, 32, 8, 0, 1, out.ctypes.data, BF16, 8, None) == INVALID
    # valid calls: a status without a device, DHR_OK with one
    if not torch.cuda.is_available():
        for name, call in calls.items():
            extra = dict(gh_dtype=BF16, gw_dtype=BF16, gb_dtype=BF16, bias_dtype=BF16) if name == "dhr_lexical_proj_backward" else {}
            assert call(value_dtype=BF16, **extra) == _lib.ERR_HIP, name
        return
    assert calls["dhr_lexical_head"](value_dtype=BF16) == OK                                       # host memory: staged by element size
    assert np.array_equal(val, np.full((2, 8), 1 / 32, np.float16)) and not idx.any()
    t, p = _device_args()
    proj = dict(hidden=p["hid"], weight=p["W"], bias=p["bias"], bias_dtype=BF16, w=p["w"], m=p["m"], ws=p["ws"], value_dtype=BF16)
    assert calls["dhr_lexical_head_train"](logits=p["lg"], w=p["w"], m=p["m"], reps=p["reps"], tok=p["tok"], ws=p["ws"], value_dtype=BF16) == OK
    assert calls["dhr_lexical_head_backward"](logits=p["lg"], g=p["g"], tok=p["tok"], ws=p["ws"], dx=p["dx"], dw=p["dw"], value_dtype=BF16) == OK
    torch.cuda.synchronize()
    assert torch.equal(t["reps"], torch.full((2, 32), 1 / 32, device="cuda")) and not t["tok"].any() and not t["dx"][:, 0].any()
    assert calls["dhr_lexical_proj_head"](**proj, ld_batch=64, val=p["val"], idx=p["idx"]) == OK
    assert calls["dhr_lexical_proj_train"](**proj, reps=p["reps"], tok=p["tok"], pwin=p["pwin"]) == OK
    assert calls["dhr_lexical_proj_backward"](**proj, g=p["g"], tok=p["tok"], pwin=p["pwin"], gh=p["gh"], gh_dtype=BF16, gw=p["gw"], gw_dtype=BF16,
                                              gb=p["gb"], gb_dtype=BF16, gtw=p["dw"]) == OK
    torch.cuda.synchronize()
    assert torch.equal(t["reps"], torch.full((2, 32), 1 / 32, device="cuda")) and torch.equal(t["pwin"], t["reps"]) and not t["gh"][:, 0].any()


def test_wrappers_raise_before_touching_the_library(monkeypatch):
    import torch
    from dhr_amd import lexical as LX
    from dhr_amd import lexical_proj as LP
    from dhr_amd import lexical_proj_train as LPT
    from dhr_amd import lexical_train as LT

    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", no_library)
    bf, f16 = torch.bfloat16, torch.float16
    lg, w, m = torch.zeros((2, 4, 32), dtype=bf), torch.ones((2, 4)), torch.ones((2, 4), dtype=torch.long)
    h, W, b = torch.zeros((2, 4, 16), dtype=bf), torch.zeros((32, 16), dtype=bf), torch.zeros((32,), dtype=bf)
    rec, idx = torch.zeros((2, 8), dtype=f16), torch.zeros((2, 8), dtype=torch.uint8)
    # a bf16 tensor on the CPU passes the dtype check and meets the device check
    for call in (lambda: LX.lexical_reps(lg, w, m), lambda: LX.densify_lexical_into(lg, w, m, rec, idx, 8, 0), lambda: LT.lexical_reps(lg, w, m),
                 lambda: LP.lexical_reps(h, W, b, w, m), lambda: LP.densify_lexical_into(h, W, b, w, m, rec, idx, 8, 0),
                 lambda: LPT.lexical_reps(h, W, b, w, m), lambda: LPT.lexical_reps(h, W.float(), None, w, m), lambda: LPT.lexical_reps(h.float(), W, b.float(), w, m)):
        with pytest.raises(_lib.DhrError, match="GPU"):
            call()
    # one fp16 and one bf16 operand: no common 16-bit type
    for call in (lambda: LP.lexical_reps(h.to(f16), W, b, w, m), lambda: LP.lexical_reps(h, W.to(f16), b, w, m),
                 lambda: LPT.lexical_reps(h.to(f16), W, b, w, m), lambda: LPT.lexical_reps(h, W.to(f16), b, w, m)):
        with pytest.raises(_lib.DhrError):
            call()
    with pytest.raises(_lib.DhrError, match="float16 and one bfloat16"):
        LPT.lexical_reps(h.to(f16), W, b, w, m)
    # float64 still is no dtype of theirs
    for call in (lambda: LX.lexical_reps(lg.double(), w, m), lambda: LT.lexical_reps(lg.double(), w, m), lambda: LP.lexical_reps(h.double(), W.double(), b, w, m),
                 lambda: LPT.lexical_reps(h.double(), W, b, w, m), lambda: LPT.lexical_reps(h, W, b.double(), w, m)):
        with pytest.raises(_lib.DhrError):
            call()
    with pytest.raises(_lib.DhrError, match="unsupported logits dtype"):
        LX.lexical_reps(lg.double().numpy(), w.numpy(), m.numpy())


def test_golden_inputs_are_bf16_values():
    n = 0
    for path in GOLD.values():
        g = np.load(path)
        for key in g.files:
            if key.endswith(("_logits", "_hidden", "_W", "_bias")):
                x = g[key].astype(np.float32)
                assert np.array_equal(rb(x), x, equal_nan=True), (path, key)
                n += 1
    assert n == 4 + 3 + 4 * 3 + 3 * 3


def test_seeds_keep_the_truth_inside_the_near_tie_cap():
    for B, T, V, seed in LOGITS:
        full, w, mask, G = logits_case(B, T, V, seed)
        near = forward64(full[:, 1:], w, mask)[4]
        assert near.sum() <= 1e-4 * B * V, (B, T, V, seed, int(near.sum()))
        assert np.array_equal(rb(full), full) and (mask[0] == 1).all() and (w < 0).any() and (w > 0).any() and (G == 0).any()
    for B, T, V, H, seed in RANDOM:
        hidden, W, bias, w, mask, G = random_case_bf16(B, T, V, H, seed)
        assert np.array_equal(rb(hidden), hidden) and np.array_equal(rb(W), W)
        for bb in (bias, None):
            x = hidden[:, 1:].astype(np.float64) @ W.astype(np.float64).T + (0 if bb is None else bb.astype(np.float64))
            near = forward64(x, w, mask)[4]
            assert near.sum() <= 1e-4 * B * V, (B, T, V, H, seed, int(near.sum()))


# ------------------------------------------------------------------------------------------ GPU part
def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _np(t):
    return t.detach().float().cpu().numpy()


def _bits(t):
    import torch
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same(x, y, what):
    import torch
    assert (x is None) == (y is None), what
    assert x is None or (x.dtype == y.dtype and torch.equal(_bits(x), _bits(y))), what


def _run_logits(full, w, mask, G, dtype, skip=1, view=False, strided=False, need=(True, True)):
    """forward + backward of lexical_train on numpy operands -> (reps, tok, dlogits [B, L, V], dw [B, T, 1])"""
    import torch
    from dhr_amd import lexical_train as LT
    B, L, V = full.shape
    if strided:
        leaf = torch.zeros((B + 1, L + 2, V + 6), dtype=dtype, device="cuda")
        leaf[1:, 1:L + 1, 2:V + 2] = _dev(full, dtype)
        leaf.requires_grad_(need[0])
        x = leaf[1:, 1:L + 1, 2:V + 2]
    else:
        leaf = _dev(full, dtype).requires_grad_(need[0])
        x = leaf
    wt = _dev(w)[..., None].requires_grad_(need[1])
    out, tok = LT.lexical_reps(x[:, skip:] if view else x, wt, _dev(mask), skip_tokens=0 if view else skip, return_tokens=True)
    out.backward(_dev(G))
    g = leaf.grad
    if strided and g is not None:
        inner = g[1:, 1:L + 1, 2:V + 2]
        assert int((g != 0).sum()) == int((inner != 0).sum())                     # nothing is written outside the view
        g = inner.contiguous()
    return out.detach(), tok, g, wt.grad


def _run_proj(hidden, W, bias, w, mask, G, dtype, skip=1, view=False, w_dtype=None, b_dtype=None, need=(True, True, True, True)):
    """forward + backward of lexical_proj_train on numpy operands -> (reps, tok, dhidden [B, L, H], dW, dbias, dw [B, T, 1])"""
    from dhr_amd import lexical_proj_train as LPT
    h = _dev(hidden, dtype).requires_grad_(need[0])
    Wt = _dev(W, w_dtype or dtype).requires_grad_(need[1])
    bt = None if bias is None else _dev(bias, b_dtype).requires_grad_(need[2])
    wt = _dev(w)[..., None].requires_grad_(need[3])
    out, tok = LPT.lexical_reps(h[:, skip:] if view else h, Wt, bt, wt, _dev(mask), skip_tokens=0 if view else skip, return_tokens=True)
    out.backward(_dev(G))
    return out.detach(), tok, h.grad, Wt.grad, None if bt is None else bt.grad, wt.grad


def _check_proj(tag, t, mask, dh, dW, db, dw, out_h="bf16", out_W="bf16", out_b=None, rows=None):
    rows = slice(None) if rows is None else rows
    res = {"dhidden": within(_np(dh), t["dh"], t["b_dh"], tag + ": proj dhidden", out_h),
           "dW": within(_np(dW)[rows], t["dW"][rows], t["b_dW"][rows], tag + ": proj dW", out_W),
           "dL/dw": within(_np(dw)[..., 0], t["dw"], t["b_dw"], tag + ": proj dL/dw")}
    if db is not None:
        res["dbias"] = within(_np(db), t["db"], t["b_db"], tag + ": proj dbias", out_b)
    assert not _np(dh)[mask == 0].any() and not _np(dw)[..., 0][mask == 0].any(), tag
    return res


@pytest.mark.gpu
def test_goldens_forward_bit_identical_to_fp16():
    import torch
    from dhr_amd import lexical as LX
    from dhr_amd import lexical_proj as LP
    from dhr_amd import lexical_proj_train as LPT
    from dhr_amd import lexical_train as LT
    bf, f16 = torch.bfloat16, torch.float16

    def records(head, args16, argsbf, B, dims, remove, agg, cls, what):
        for a in (args16, argsbf):
            a["rep"] = head.lexical_reps(*a["in"])
        _same(args16["rep"], argsbf["rep"], what + " reps")
        nc = cls.shape[1]
        if dims:
            for a in (args16, argsbf):
                a["rv"], a["ri"] = torch.full((B, dims + nc), 7.0, dtype=f16, device="cuda"), torch.full((B, dims), 99, dtype=torch.uint8, device="cuda")
                head.densify_lexical_into(*a["in"], a["rv"], a["ri"], dims, remove, semantic_reps=cls)
            _same(args16["rv"], argsbf["rv"], what + " densified values")
            _same(args16["ri"], argsbf["ri"], what + " densified groups")
        for full in (True, False):
            for a in (args16, argsbf):
                a["av"] = torch.full((B, agg + nc), 7.0, dtype=f16, device="cuda")
                head.aggregate_lexical_into(*a["in"], a["av"], agg, full=full, semantic_reps=cls)
            _same(args16["av"], argsbf["av"], f"{what} aggregate(full={full})")
        return args16["rep"]

    g = np.load(GOLD["lexical"])
    for name in ("prod", "small", "neg", "pad"):
        lg, w, mk, cls = g[name + "_logits"], _dev(g[name + "_w"]), _dev(g[name + "_mask"])[:, 1:], _dev(g[name + "_cls"])
        B = lg.shape[0]
        dims, remove = (int(v) for v in g[name + "_geom"][:2]) if name + "_geom" in g else (0, 0)
        agg = 640 if name == "prod" else 700 if name == "pad" else 8
        rep = records(LX, {"in": (_dev(lg)[:, 1:], w, mk)}, {"in": (_dev(lg, bf)[:, 1:], w, mk)}, B, dims, remove, agg, cls, "lexical " + name)
        assert np.allclose(rep.cpu().numpy(), g[name + "_reps"], rtol=1e-5, atol=1e-30)          # (what test_lexical_head.py holds the fp16 call to)
    # the staged host path through ctypes: the bf16 bits in a uint16 numpy array
    lg = g["small_logits"][:, 1:]
    B, T, V = lg.shape
    bits = np.ascontiguousarray(_dev(lg, bf).view(torch.int16).cpu().numpy().view(np.uint16))
    w, m, out = np.ascontiguousarray(g["small_w"]), np.ascontiguousarray(g["small_mask"][:, 1:].astype(np.float32)), np.zeros((B, V), np.float32)
    rc = _head(_lib.load(), mem_kind=_lib.MEM_HOST, mode=_lib.LEX_RAW, logits=bits.ctypes.data, value_dtype=_lib.VAL_BF16, batch=B, n_tokens=T, vocab=V,
               ld_batch=T * V, ld_token=V, w=w.ctypes.data, ld_w=T, m=m.ctypes.data, ld_m=T, dims=0, val=out.ctypes.data, val_dtype=_lib.VAL_F32, ld_val=V)
    assert rc == _lib.DHR_OK
    dev16 = LX.lexical_reps(_dev(lg), _dev(g["small_w"]), _dev(g["small_mask"])[:, 1:])
    assert np.array_equal(out.view(np.uint32), dev16.cpu().numpy().view(np.uint32))

    g = np.load(GOLD["lexical_train"])
    for name in ("prod", "small", "neg"):
        lg, w, mk = g[name + "_logits"], _dev(g[name + "_w"]), _dev(g[name + "_mask"])[:, 1:]
        r16, t16 = LT.lexical_reps(_dev(lg), w, mk, skip_tokens=1, return_tokens=True)
        rbf, tbf = LT.lexical_reps(_dev(lg, bf), w, mk, skip_tokens=1, return_tokens=True)
        _same(r16, rbf, "lexical_train reps " + name)
        _same(t16, tbf, "lexical_train tok " + name)

    g = np.load(GOLD["lexical_proj"])
    for name in ("prod", "small", "neg", "pad"):
        hid, W, bias = g[name + "_hidden"], g[name + "_W"], g[name + "_bias"]
        w, mk, cls = _dev(g[name + "_w"]), _dev(g[name + "_mask"])[:, 1:], _dev(g[name + "_cls"])
        dims, remove, agg = (int(v) for v in g[name + "_geom"])
        for b16, bbf in ((_dev(bias), _dev(bias)), (_dev(bias, f16), _dev(bias, bf)), (None, None), (_dev(bias, bf), _dev(bias, f16))):
            records(LP, {"in": (_dev(hid)[:, 1:], _dev(W), b16, w, mk)}, {"in": (_dev(hid, bf)[:, 1:], _dev(W, bf), bbf, w, mk)}, hid.shape[0], dims,
                    remove, agg, cls, "lexical_proj " + name)

    g = np.load(GOLD["lexical_proj_train"])
    for name in ("prod", "small", "neg"):
        hid, W, bias, w, mk = g[name + "_hidden"], g[name + "_W"], _dev(g[name + "_bias"]), _dev(g[name + "_w"]), _dev(g[name + "_mask"])[:, 1:]
        r16, t16 = LPT.lexical_reps(_dev(hid), _dev(W), bias, w, mk, skip_tokens=1, return_tokens=True)
        rbf, tbf = LPT.lexical_reps(_dev(hid, bf), _dev(W, bf), bias, w, mk, skip_tokens=1, return_tokens=True)
        _same(r16, rbf, "lexical_proj_train reps " + name)
        _same(t16, tbf, "lexical_proj_train tok " + name)
        _same(rbf, LP.lexical_reps(_dev(hid, bf)[:, 1:], _dev(W, bf), bias, w, mk), "training and encoding forward " + name)


@pytest.mark.gpu
def test_goldens_backward_within_the_bounds():
    import torch
    bf, f16 = torch.bfloat16, torch.float16
    g = np.load(GOLD["lexical_train"])
    for name in ("prod", "small", "neg"):
        lg, w, m, G, dlg, dw = (g[name + k] for k in ("_logits", "_w", "_mask", "_G", "_dlogits", "_dw"))
        m = m[:, 1:]
        p, d, r, a, near, c = forward64(lg[:, 1:], w, m)
        out, tok, gx, gw = _run_logits(lg, w, m, G, bf)
        out16, tok16, gx16, gw16 = _run_logits(lg, w, m, G, f16)
        assert gx.dtype == bf and gx.shape == lg.shape and np.array_equal(tok.cpu().numpy(), a), name
        _same(gw, gw16, name + " dL/dw of lexical_train")                         # fp32 from fp32: never sees a 16-bit rounding
        gxn = _np(gx)
        assert not gxn[:, 0].any() and not gxn[:, 1:][m == 0].any() and not _np(gw)[..., 0][m == 0].any(), name
        dx64, b_dx, dw64, b_dw = backward64(p, d, w, m, G, a)
        within(gxn[:, 1:], dx64, b_dx, f"golden {name}: logits dL/dlogits", "bf16")
        within(_np(gw)[..., 0], dw64, b_dw, f"golden {name}: logits dL/dw")
        # ... and against what the reference's autograd returned, each within the bound of the truth
        assert np.all(np.abs(gxn[:, 1:] - dlg[:, 1:]) <= 2 * b_dx + np.where(dlg[:, 1:] != 0, np.maximum(UB16 * np.abs(dlg[:, 1:]), SUBB16), 0))
        assert np.all(np.abs(_np(gw)[..., 0] - dw) <= 2 * b_dw)
    g = np.load(GOLD["lexical_proj_train"])
    for name in ("prod", "small", "neg"):
        hid, W, bias, w, mask, G = (g[name + k] for k in ("_hidden", "_W", "_bias", "_w", "_mask", "_G"))
        mask = mask[:, 1:]
        out, tok, dh, dW, db, dw = _run_proj(hid, W, bias, w, mask, G, bf)
        t = truth64(hid[:, 1:], W, bias, w, mask, G, tok=tok.cpu().numpy(), what=name)       # exact-arithmetic operands: nothing is widened
        assert t["ties"] == 0 and np.array_equal(tok.cpu().numpy(), t["a"]), name
        assert dh.dtype == bf and dW.dtype == bf and db.dtype == torch.float32 and dh.shape == hid.shape and not dh[:, 0].any()
        rows = g[name + "_dW_rows"]
        _check_proj("golden " + name, t, mask, dh[:, 1:], dW, db, dw)
        f = truth64(hid[:, 1:], W, bias, w, mask, G, u16=0)                                   # the reference's fp32 autograd keeps dx in fp32
        r16 = lambda x: np.where(x != 0, np.maximum(UB16 * np.abs(x), SUBB16), 0)             # noqa: E731
        assert np.all(np.abs(_np(dh)[:, 1:] - g[name + "_dhidden"][:, 1:]) <= t["b_dh"] + f["b_dh"] + r16(g[name + "_dhidden"][:, 1:]))
        assert np.all(np.abs(_np(dW)[rows] - g[name + "_dW"]) <= (t["b_dW"] + f["b_dW"])[rows] + r16(g[name + "_dW"]))
        assert np.all(np.abs(_np(db) - g[name + "_dbias"]) <= t["b_db"] + f["b_db"])
        assert np.all(np.abs(_np(dw)[..., 0] - g[name + "_dw"]) <= 2 * t["b_dw"])
    print("worst error / bound:", {k: round(v, 4) for k, v in sorted(WORST.items())})


@pytest.mark.gpu
def test_range_of_bf16_is_kept():
    import torch
    from dhr_amd import lexical as LX
    bf = torch.bfloat16
    g = np.load(GOLD["lexical_proj_train"])
    up, down = 2.0 ** 40, 2.0 ** -40
    for name in ("small", "neg"):
        hid, W, bias, w, mask, G = (g[name + k].astype(np.float32) if g[name + k].dtype == np.float16 else g[name + k]
                                    for k in ("_hidden", "_W", "_bias", "_w", "_mask", "_G"))
        mask = mask[:, 1:]
        assert np.array_equal(rb(hid * up), hid * up) and np.array_equal(rb(W * down), W * down)           # exact in bf16, far outside fp16
        assert np.abs(hid * up).max() > 65504 and np.abs((W * down)[W != 0]).max() < 2.0 ** -24
        base = _run_proj(hid, W, bias, w, mask, G, bf)
        scaled = _run_proj(hid * np.float32(up), W * np.float32(down), bias, w, mask, G, bf)
        _same(base[0], scaled[0], name + " reps")
        _same(base[1], scaled[1], name + " tok")
        _same(base[2], (scaled[2].float() * up).to(bf), name + " dhidden * 2^40")
        assert torch.equal(scaled[2].float() * up, base[2].float()), name
        _same(base[3], (scaled[3].float() * down).to(bf), name + " dW * 2^-40")
        assert torch.equal(scaled[3].float() * down, base[3].float()), name
        _same(base[4], scaled[4], name + " dbias")
        _same(base[5], scaled[5], name + " dL/dw")
        assert base[2].any() and base[3].any()
    # the logits heads: one token row of +-2^100
    B, T, V, seed = LOGITS[3]
    full, w, mask, G = logits_case(B, T, V, seed)
    sign = np.where(np.random.default_rng(5).random(V) < 0.5, -1.0, 1.0).astype(np.float32)
    full[0, 4] = sign * np.float32(2.0 ** 100)
    mask[:] = 1
    w[0, 3] = 50.0                                                                 # ... which wins its columns: the row takes gradient
    assert np.array_equal(rb(full), full)
    p, d, r, a, near, c = forward64(full[:, 1:], w, mask)
    assert (p[0, 3][sign > 0] > 0).all() and not p[0, 3][sign < 0].any() and (a[0] == 3).any()
    out, tok, gx, gw = _run_logits(full, w, mask, G, bf)
    _same(out, LX.lexical_reps(_dev(full, bf)[:, 1:], _dev(w), _dev(mask)), "2^100: encoding and training forward")
    assert check_routing(tok.cpu().numpy(), a, near, c, "2^100 row") <= 1e-4 * B * V and np.all(np.abs(_np(out) - r) <= RTOL * np.abs(r) + ATOL)
    dx64, b_dx, dw64, b_dw = backward64(p, d, w, mask, G, tok.cpu().numpy())
    within(_np(gx)[:, 1:], dx64, b_dx, "2^100 row: logits dL/dlogits", "bf16")
    within(_np(gw)[..., 0], dw64, b_dw, "2^100 row: logits dL/dw")
    assert np.isfinite(_np(gx)).all() and _np(gx)[0, 4].any()


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,V,seed", LOGITS)
def test_random_logits_against_the_float64_truth(B, T, V, seed):
    import torch
    from dhr_amd import lexical as LX
    bf = torch.bfloat16
    full, w, mask, G = logits_case(B, T, V, seed)
    tag = f"random logits {B}x{T}x{V}"
    whole = _run_logits(full, w, mask, G, bf)
    for other, what in ((_run_logits(full, w, mask, G, bf, view=True), "the [:, 1:] view"), (_run_logits(full, w, mask, G, bf, strided=True), "a row-strided view")):
        for x, y in zip(whole, other):
            _same(x, y, f"{tag}: {what}")
    out, tok, gx, gw = whole
    _same(out, LX.lexical_reps(_dev(full, bf)[:, 1:], _dev(w), _dev(mask)), tag + ": the encoding head")
    p, d, r, a, near, c = forward64(full[:, 1:], w, mask)
    ties = check_routing(tok.cpu().numpy(), a, near, c, tag)
    assert ties <= 1e-4 * B * V, tag
    assert np.all(np.abs(_np(out) - r) <= RTOL * np.abs(r) + ATOL), tag
    gxn = _np(gx)
    assert gx.dtype == bf and not gxn[:, 0].any() and not gxn[:, 1:][mask == 0].any() and not _np(gw)[..., 0][mask == 0].any(), tag
    dx64, b_dx, dw64, b_dw = backward64(p, d, w, mask, G, tok.cpu().numpy())
    rx = within(gxn[:, 1:], dx64, b_dx, tag + ": logits dL/dlogits", "bf16")
    rw = within(_np(gw)[..., 0], dw64, b_dw, tag + ": logits dL/dw")
    print(f"{tag}: {ties} near-ties; worst error / bound dL/dlogits {rx:.4f}, dL/dw {rw:.4f}")


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,V,H,seed", RANDOM)
def test_random_projection_cases_against_the_float64_truth(B, T, V, H, seed):
    import torch
    from dhr_amd import lexical_proj as LP
    bf = torch.bfloat16
    hidden, W, bias, w, mask, G = random_case_bf16(B, T, V, H, seed)
    tag = f"random {B}x{T}x{V}x{H}"
    whole = _run_proj(hidden, W, bias, w, mask, G, bf)
    for x, y in zip(whole, _run_proj(hidden, W, bias, w, mask, G, bf, view=True)):
        _same(x, y, tag + ": the [:, 1:] view")
    out, tok, dh, dW, db, dw = whole
    _same(out, LP.lexical_reps(_dev(hidden, bf)[:, 1:], _dev(W, bf), _dev(bias), _dev(w), _dev(mask)), tag + ": the encoding head")
    t = truth64(hidden[:, 1:], W, bias, w, mask, G, tok=tok.cpu().numpy(), inexact=True, what=tag)
    assert t["ties"] <= 1e-4 * B * V, tag
    assert not dh[:, 0].any() and not dh[-1].any() and dh.dtype == bf and dW.dtype == bf and db.dtype == torch.float32
    res = _check_proj(tag + " bias", t, mask, dh[:, 1:], dW, db, dw)
    out0, tok0, dh0, dW0, db0, dw0 = _run_proj(hidden, W, None, w, mask, G, bf)
    t = truth64(hidden[:, 1:], W, None, w, mask, G, tok=tok0.cpu().numpy(), inexact=True, what=tag + " no bias")
    assert t["ties"] <= 1e-4 * B * V and db0 is None and not dh0[:, 0].any(), tag
    res0 = _check_proj(tag + " no bias", t, mask, dh0[:, 1:], dW0, None, dw0)
    print(f"{tag}: worst error / bound with a bias {res}, without {res0}")


@pytest.mark.gpu
def test_operand_rule_and_gradient_subsets():
    import torch
    bf, f16, f32 = torch.bfloat16, torch.float16, torch.float32
    B, T, V, H, seed = 6, 50, 1030, 136, 21
    hidden, W, bias, w, mask, G = random_case_bf16(B, T, V, H, seed)
    W32 = (np.random.default_rng(seed + 1).standard_normal((V, H)) * (2 / np.sqrt(H))).astype(np.float32)      # an fp32 master weight: no bf16 values
    assert not np.array_equal(rb(W32), W32)
    ref = _run_proj(hidden, rb(W32), bias, w, mask, G, bf)                         # the caller rounds the weight to bf16
    got = _run_proj(hidden, W32, bias, w, mask, G, bf, w_dtype=f32)                # the op rounds it, once
    for k, (x, y) in enumerate(zip(ref, got)):
        if k == 3:
            assert y.dtype == f32 and x.dtype == bf                               # dW in the master weight's dtype; the same fp32 sums rounded once more
            _same(x, y.to(bf), "dW")
        else:
            _same(x, y, f"output {k} with an fp32 weight")
    got = _run_proj(hidden, W, bias, w, mask, G, f32, w_dtype=bf)                  # fp32 hidden states (bf16 values), bf16 weight
    base = _run_proj(hidden, W, bias, w, mask, G, bf)
    assert got[2].dtype == f32 and got[3].dtype == bf
    for k in (0, 1, 3, 4, 5):
        _same(base[k], got[k], f"output {k} with fp32 hidden states")
    _same(base[2], got[2].to(bf), "dhidden")
    # the bias: bf16 in, bf16 out, rounded once from the fp32 sum that an fp32 bias gets back
    withb = _run_proj(hidden, W, rb(bias), w, mask, G, bf, b_dtype=bf)
    plain = _run_proj(hidden, W, rb(bias), w, mask, G, bf)
    assert withb[4].dtype == bf and plain[4].dtype == f32
    _same(withb[4], plain[4].to(bf), "dbias")
    for k in (0, 1, 2, 3, 5):
        _same(withb[k], plain[k], f"output {k} with a bf16 bias")
    # an fp16 bias next to bf16 operands keeps its own dtype
    b16 = bias.astype(np.float16)
    half = _run_proj(hidden, W, b16, w, mask, G, bf, b_dtype=f16)
    wide = _run_proj(hidden, W, b16.astype(np.float32), w, mask, G, bf)
    assert half[4].dtype == f16 and half[2].dtype == bf and wide[4].dtype == f32
    _same(half[4], wide[4].to(f16), "dbias in fp16 from the bf16 kernels")
    for k in (0, 1, 2, 3, 5):
        _same(half[k], wide[k], f"output {k} with an fp16 bias next to bf16 operands")
    # gradient subsets: what is still computed has the same bits
    for need in ((True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True),
                 (True, False, True, True), (False, True, True, True)):
        sub = _run_proj(hidden, W, bias, w, mask, G, bf, need=need)[2:]
        for wanted, x, y in zip(need, sub, base[2:]):
            assert (x is not None) == wanted, need
            if wanted:
                _same(x, y, f"subset {need}")
    # the logits head: a frozen term weight, detached logits
    full, w, mask, G = logits_case(*LOGITS[0])
    both = _run_logits(full, w, mask, G, bf)
    _same(both[2], _run_logits(full, w, mask, G, bf, need=(True, False))[2], "dL/dlogits alone")
    _same(both[3], _run_logits(full, w, mask, G, bf, need=(False, True))[3], "dL/dw alone")


@pytest.mark.gpu
def test_two_runs_are_bit_identical():
    import torch
    from dhr_amd import lexical as LX
    from dhr_amd import lexical_proj as LP
    bf = torch.bfloat16
    full, w, mask, G = logits_case(*LOGITS[1])
    runs = [_run_logits(full, w, mask, G, bf) for _ in range(2)]
    for x, y in zip(*runs):
        _same(x, y, "lexical_train")
    enc = [LX.lexical_reps(_dev(full, bf)[:, 1:], _dev(w), _dev(mask)) for _ in range(2)]
    _same(enc[0], enc[1], "lexical")
    hidden, W, bias, w, mask, G = random_case_bf16(6, 50, 1030, 136, 21)
    runs = [_run_proj(hidden, W, bias, w, mask, G, bf, b_dtype=bf) for _ in range(2)]
    for x, y in zip(*runs):
        _same(x, y, "lexical_proj_train")
    rec = []
    for _ in range(2):
        rv, ri = torch.zeros((6, 64), dtype=torch.float16, device="cuda"), torch.zeros((6, 64), dtype=torch.uint8, device="cuda")
        LP.densify_lexical_into(_dev(hidden, bf)[:, 1:], _dev(W, bf), _dev(bias, bf), _dev(w), _dev(mask), rv, ri, 64, 6)
        rec.append((rv, ri))
    _same(rec[0][0], rec[1][0], "lexical_proj values")
    _same(rec[0][1], rec[1][1], "lexical_proj groups")


@pytest.mark.gpu
def test_composed_step_under_bf16_autocast():
    """A toy encoder as bf16 training runs it: the hidden states are the bf16 output of a layer norm, the projector keeps an fp32 master weight
    and an fp32 bias, and the step is lexical_proj_train.lexical_reps -> listwise_gip_scores -> dhr_loss -> backward inside torch.autocast.  The
    op reads the master weight rounded to bf16 once (what autocast's linear would multiply), so the truth is the float64 restatement on those
    bf16 operand values with the step's own dL/dreps and routing.  Held to it: dL/dhidden (bf16), dL/dW and dL/dbias (fp32, the master copies'
    dtype), dL/dw of the term weights, and the layer norm's weight and bias gradients.  The last two are torch's fp32 layer-norm backward of
    dL/dhidden (the semantic scores are constants here, so nothing else reaches the states): with xhat the normalised states in float64,
    dbeta = sum_rows dy and dgamma = sum_rows dy xhat, and with E = b_dh + the bf16 rounding of dL/dhidden, the bound of each entry of dy,
        |dbeta - truth|  <= sum E + N u sum (|dy| + E)                                       N = the rows added up, in fp32, in any order
        |dgamma - truth| <= sum E |xhat| + sum (|dy| + E) d + N u sum (|dy| + E) (|xhat| + d)
    where d = (4 H + 16) u (|xhat| + max_k |x_k| rstd) bounds the fp32 evaluation of xhat: the mean and the variance are fp32 sums of H terms
    (H u each, the variance of squares of differences that carry the mean's error twice), the square root, the difference and the product
    a few u more.  Each plus one rounding of the sum of the two sides' gradients.  The gradient of the input embeddings is not checked: it is the
    same backward once more and belongs to no parameter."""
    import torch
    from dhr_amd import gip_scores as GS
    from dhr_amd import lexical_proj_train as LPT
    from dhr_amd import train_loss as TL
    bf = torch.bfloat16
    L, H, V, dims, remove, n_q, n_pass = 16, 64, 515, 64, 3, 2, 2
    rng = np.random.default_rng(37)
    ln = torch.nn.LayerNorm(H).cuda()                                             # fp32 parameters; autocast runs it in fp32
    with torch.no_grad():
        ln.weight.copy_(_dev(1 + 0.1 * rng.standard_normal(H).astype(np.float32)))
        ln.bias.copy_(_dev(0.1 * rng.standard_normal(H).astype(np.float32)))
    W = _dev((rng.standard_normal((V, H)) * (2 / np.sqrt(H))).astype(np.float32)).requires_grad_(True)
    bias = _dev((rng.standard_normal(V) * 0.1).astype(np.float32)).requires_grad_(True)
    sides, kept = {}, {}
    with torch.autocast("cuda", dtype=bf):
        for side, B in (("q", n_q), ("p", n_q * n_pass)):                         # the passages: B = 4, L = 16, H = 64, V = 515
            emb = _dev(rng.standard_normal((B, L, H)).astype(np.float32)).requires_grad_(True)
            w = _dev(np.abs(rng.standard_normal((B, L - 1, 1))).astype(np.float32)).requires_grad_(True)
            mask = _dev((np.arange(L - 1)[None] < rng.integers(2, L, (B, 1))).astype(np.int64))
            h = ln(emb).to(bf)                                                     # the states as a bf16 model hands them on
            h.retain_grad()
            reps, tok = LPT.lexical_reps(h, W, bias, w, mask, skip_tokens=1, return_tokens=True)
            reps.retain_grad()
            sides[side] = (emb, h, w, mask, reps, tok)
        lexical = GS.listwise_gip_scores(sides["q"][4], sides["p"][4], n_q, dims, remove)
        semantic = _dev(rng.standard_normal((n_q, n_q * n_pass)).astype(np.float32))
        loss, _ = TL.dhr_loss(lexical, semantic, train_n_passages=n_pass, lamb=1.0)
    loss.backward()
    assert W.grad.dtype == torch.float32 and bias.grad.dtype == torch.float32 and ln.weight.grad is not None and ln.weight.grad.any()
    Wv = rb(_np(W))
    total = {"dW": np.zeros((V, H)), "b_dW": np.zeros((V, H)), "db": np.zeros(V), "b_db": np.zeros(V)}
    lnt = {k: np.zeros(H) for k in ("dgamma", "b_dgamma", "dbeta", "b_dbeta")}
    for side, (emb, h, w, mask, reps, tok) in sides.items():
        tag = f"composed {side}"
        G, mk = _np(reps.grad), mask.cpu().numpy()
        assert G.any() and emb.grad is not None and h.grad.dtype == bf
        t = truth64(_np(h)[:, 1:], Wv, _np(bias), _np(w)[..., 0], mk, G, tok=tok.cpu().numpy(), inexact=True, what=tag)
        assert t["ties"] <= 1e-4 * reps.numel(), tag
        within(_np(h.grad)[:, 1:], t["dh"], t["b_dh"], tag + ": composed dhidden", "bf16")
        within(_np(w.grad)[..., 0], t["dw"], t["b_dw"], tag + ": composed dL/dw")
        assert not _np(h.grad)[:, 1:][mk == 0].any() and not _np(h.grad)[:, 0].any()
        for k in total:
            total[k] += t[k]
        # the layer norm's parameters: dy = dL/dhidden of all L tokens (token 0: exactly zero), rows = (passage, token)
        x = _np(emb).astype(np.float64)
        mean, var = x.mean(-1, keepdims=True), x.var(-1, keepdims=True)
        rstd = 1 / np.sqrt(var + ln.eps)
        xhat = (x - mean) * rstd
        d = (4 * H + 16) * U32 * (np.abs(xhat) + np.abs(x).max(-1, keepdims=True) * rstd)
        dy = np.concatenate([np.zeros((x.shape[0], 1, H)), t["dh"]], 1)
        E = np.concatenate([np.zeros((x.shape[0], 1, H)), t["b_dh"] + np.where(t["dh"] != 0, np.maximum(UB16 * np.abs(t["dh"]), SUBB16), 0.0)], 1)
        N = x.shape[0] * L
        lnt["dbeta"] += dy.sum((0, 1))
        lnt["b_dbeta"] += E.sum((0, 1)) + N * U32 * (np.abs(dy) + E).sum((0, 1))
        lnt["dgamma"] += (dy * xhat).sum((0, 1))
        lnt["b_dgamma"] += (E * np.abs(xhat)).sum((0, 1)) + ((np.abs(dy) + E) * d).sum((0, 1)) + N * U32 * ((np.abs(dy) + E) * (np.abs(xhat) + d)).sum((0, 1))
    # W and bias are shared by the two sides: autograd adds the two fp32 gradients, one more rounding of the sum
    within(_np(W.grad), total["dW"], total["b_dW"] + U32 * np.abs(total["dW"]) + U32 * total["b_dW"], "composed: composed dW")
    within(_np(bias.grad), total["db"], total["b_db"] + U32 * np.abs(total["db"]) + U32 * total["b_db"], "composed: composed dbias")
    for got, k in ((ln.weight.grad, "dgamma"), (ln.bias.grad, "dbeta")):
        assert got.dtype == torch.float32 and got.any()
        within(_np(got), lnt[k], lnt["b_" + k] + U32 * np.abs(lnt[k]) + U32 * lnt["b_" + k], f"composed: composed layer norm {k}")
    print(f"composed step under autocast: loss {float(loss.detach()):.6f}; worst error / bound", {k: round(v, 4) for k, v in sorted(WORST.items()) if "composed" in k})


@pytest.mark.gpu
def test_memory_has_no_widened_copy():
    """B = 4, L = 65 (T = 64), V = 30522.  lexical_train on bf16 logits: over a forward plus backward, what is allocated beyond the inputs and
    the returned tensors (reps, the gradients) stays under half of ONE fp32 [B, T, V] tensor: a widened copy of the logits, or an fp32 gradient
    rounded afterwards, would be a whole one.  lexical_proj_train on bf16 operands, H = 64: the two limits of
    tests/test_lexical_proj_train.py::test_memory_has_no_btv_term at this shape, as written there -- the peak over the inputs at B = 4 stays
    under the 16-bit logits alone, and between two batch sizes it grows by at most (B2 - B1) * (16 V + 8 T H + 512 T) bytes.  The second size is
    that test's own smaller one, B = 64.  A nearer one would not do, for fp16 as for bf16: up to 16 row tiles (B = 16 here) pass 2 splits the
    vocabulary into 16 shares, and their fp32 partials of dhidden, 4 * 16 * T * H bytes per passage (262 KB), grow with B until the share
    count starts to fall; next to 10 V bytes of reps, winner and its softmax value that is 592 KB per passage against the cap's 553 KB
    (measured from B = 4 to B = 8: 2.59 MB against 2.22 MB).  From B = 16 on the partials stay at 4.2 MB and the cap holds with room; a
    [B, T, V] term would be 3.9 MB per passage, seven times the cap."""
    import torch
    from dhr_amd import lexical_proj_train as LPT
    from dhr_amd import lexical_train as LT
    bf = torch.bfloat16
    B, L, V, H = 4, 65, 30522, 64
    T = L - 1
    gen = torch.Generator(device="cuda").manual_seed(31)
    lg = (torch.randn((B, L, V), generator=gen, device="cuda") * 2).to(bf).requires_grad_(True)
    w = torch.randn((B, T, 1), generator=gen, device="cuda").requires_grad_(True)
    mask = torch.ones((B, T), dtype=torch.int64, device="cuda")
    G = torch.randn((B, V), generator=gen, device="cuda")
    LT.lexical_reps(lg, w, mask, skip_tokens=1).backward(G)                        # warm-up: the library is loaded, the kernels are resident
    lg.grad = w.grad = None
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    reps = LT.lexical_reps(lg, w, mask, skip_tokens=1)
    reps.backward(G)
    torch.cuda.synchronize()
    returned = sum(t.numel() * t.element_size() for t in (reps, lg.grad, w.grad))
    extra = torch.cuda.max_memory_allocated() - before - returned
    one_fp32 = 4 * B * T * V
    print(f"memory (lexical_train, bf16): {extra / 1e6:.2f} MB beyond the inputs and the returned tensors; one fp32 [B, T, V] tensor is {one_fp32 / 1e6:.2f} MB")
    assert lg.grad.dtype == bf and extra < one_fp32 / 2
    del lg, w, reps, G
    W = (torch.randn((V, H), generator=gen, device="cuda") * 0.25).to(bf).requires_grad_(True)
    bias = (torch.randn((V,), generator=gen, device="cuda") * 0.1).requires_grad_(True)
    peaks = {}
    for Bp in (4, 64, 4, 64):                                                       # (the first round warms the allocator)
        hidden = torch.randn((Bp, L, H), generator=gen, device="cuda").to(bf).requires_grad_(True)
        w = torch.randn((Bp, T, 1), generator=gen, device="cuda").requires_grad_(True)
        mask = torch.ones((Bp, T), dtype=torch.int64, device="cuda")
        G = torch.randn((Bp, V), generator=gen, device="cuda")
        W.grad = bias.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        LPT.lexical_reps(hidden, W, bias, w, mask, skip_tokens=1).backward(G)
        torch.cuda.synchronize()
        peaks[Bp] = torch.cuda.max_memory_allocated() - before
        del hidden, w, mask, G
    logits16 = 2 * B * T * V
    growth, cap = peaks[64] - peaks[4], 60 * (16 * V + 8 * T * H + 512 * T)
    print(f"memory (lexical_proj_train, bf16): peak over the inputs {peaks[4] / 1e6:.2f} MB at B = 4, {peaks[64] / 1e6:.2f} MB at B = 64 (the 16-bit logits "
          f"alone at B = 4: {logits16 / 1e6:.2f} MB); growth {growth / 1e6:.2f} MB, cap {cap / 1e6:.2f} MB")
    assert peaks[4] < logits16
    assert growth <= cap
