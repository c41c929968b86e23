"""The differentiable lexical head with the vocabulary projection fused in (dhr_amd/lexical_proj_train.py on dhr_lexical_proj_train /
dhr_lexical_proj_backward, dhr_amd/csrc/lexical_proj_train.hip) against the reference's own encoder code under autograd
(tests/golden/lexical_proj_train_golden.npz, made by tests/golden/make_golden_lexical_proj_train.py), a float64 restatement, and the parent
composition on the same device: torch.nn.functional.linear in fp16, dhr_amd.lexical_train.lexical_reps, .backward().

Tolerances are derived, not picked.  softmax64 / forward64 / backward64 / check_routing / assert_within are those of tests/test_lexical_train.py
(read its docstring for kappa, b_dx and b_dw); u = 2^-24.  With x the float64 logits of the fp16 operand VALUES, dx the float64 gradient of
the logits under the library's routing and b_dx, b_dw the bounds of backward64:
 - exact-arithmetic operands (the goldens, the production geometry): every evaluation of x is exact, nothing is widened;
 - inexact operands: the fp32 accumulation of x is off by at most (H + 1) u A[b][t], A = max_v (sum_k |h||W| + |bias|) as in
   tests/test_lexical_proj.py, and the normaliser by as much again relatively, so kappa (and kr) grow by 2 (H + 2) A[b][t] units of u:
   b_dx += 2 * 2 (H + 2) A u p (|R| + S1), b_dw += 2 (H + 2) A u |m| sum |g p|  (both bounds are linear in kappa and kr);
 - the second products take dx rounded to fp16 once: that operand is off by  e = b_dx + max(2^-11 |dx|, 2^-25)  (e = 0 where dx and b_dx are
   both zero: masked rows are never formed, and a live row without a routed column is p * (0 - 0));
 - fp32 accumulation of n terms in any order is off by at most n u sum |terms|:
       |dhidden - truth| <= sum_v e |W| + V u sum_v (|dx| + e) |W|
       |dW - truth|      <= sum_r e |h| + M u sum_r (|dx| + e) |h|            M = the unmasked token rows
       |dbias - truth|   <= sum_r b_dx + M u sum_r |dx|                       (the library adds the unrounded dx)
       dL/dw within b_dw
   each plus the rounding of an fp16 output, 2^-11 |truth| (2^-25 below the normal range).  Where truth and bound are zero the result must be
   exactly zero.
The reference's fp32 autograd (the fixture) keeps dx in fp32: e = b_dx there.  The parent composition rounds dx to fp16 BEFORE its bias
gradient adds it up, so its dbias is held to sum_r e + M u sum_r (|dx| + e); everything else of it is held to the bounds above.
Routing: tok equals the float64 first-argmax outside counted near-ties (zero on the goldens, at most 1e-4 of the (b, v) entries on random
data; the seeds below keep the float64 truth itself inside that cap, which the CPU part asserts).

Random data is drawn with numpy on the CPU from fixed seeds, so the truth is the same on every machine.  Measured worst error / bound on an
MI355X: profiles/lexical_proj_train.txt.

CPU part (-m "not gpu"): fixture vs restatement, symbols, workspace bound, statuses of both entry points, the wrapper's errors, the near-tie
cap of the seeds.  GPU part: -m gpu."""
import fnmatch
import os
import re

import numpy as np
import pytest

from dhr_amd import _lib
from tests.test_lexical_train import SUB16, U16, U32, assert_within, backward64, check_routing, forward64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lexical_proj_train_golden.npz")
CASES = ("prod", "small", "neg")
NEW = ("dhr_lexical_proj_train_workspace", "dhr_lexical_proj_train", "dhr_lexical_proj_backward")
# B, T, V, H, seed: what each exercises in this implementation (pass 2 splits the vocabulary where the list has at most 128 row tiles)
RANDOM = [
    (5, 70, 762, 72, 11),     # ragged masks; passages straddling 64-row tiles; V = 2 * 256 + 250; H = 64 + 8; 6 row tiles: 3 vocabulary shares
    (3, 150, 1030, 768, 12),  # full H (12 chunks in registers); four vocabulary tiles plus a 6-column tail; 8 row tiles: 5 vocabulary shares
    (33, 40, 515, 64, 13),    # many row tiles (21, of 3 shares); five token tiles per weight-gradient workgroup
    (2, 9, 202, 24, 14),      # M < 64, V < 256: one row tile, one vocabulary tile (a single share)
    (130, 64, 515, 64, 15),   # 130 row tiles: the unsplit dhidden path, straight into the output
    (6, 50, 1030, 136, 16),   # H = 2 * 64 + 8: three chunks, the six-chunk instantiation of both gradient kernels, its last chunk partial
    (3, 20, 515, 776, 16),    # H above 768: two slabs of 7 + 6 chunks, the last chunk 8 columns; M < 64: one row tile, 3 vocabulary shares
    (4, 40, 1030, 1024, 16),  # the widest H: two slabs of 8 chunks; 3 row tiles, 5 vocabulary shares written by two launches, one combine
    (130, 64, 300, 800, 16),  # H above 768 on the unsplit path: each slab stores its columns of dhidden straight into the output
]


def _golden():
    return np.load(GOLDEN)


def _ws_bound(B, T, H):
    return 256 * B * T + 65536 * H + 65536


def _exact_logits(hidden, W, bias):
    """float64 logits of exact-arithmetic operands, after asserting the recipe's promise (tests/test_lexical_proj.py)"""
    x = hidden.astype(np.float64) @ W.astype(np.float64).T + (0 if bias is None else bias.astype(np.float64))
    x32 = hidden.astype(np.float32) @ W.astype(np.float32).T + (0 if bias is None else bias.astype(np.float32))
    assert np.array_equal(x32.astype(np.float64), x) and np.array_equal(x.astype(np.float16).astype(np.float64), x) and np.abs(x).max() < 2 ** 9
    return x


def truth64(hidden, W, bias, w, m, G, tok=None, inexact=False, dx_fp16=True, what=""):
    """The float64 restatement, passage by passage.  hidden [B, T, H], W [V, H], bias [V] or None: the VALUES the kernels read; tok: the
    library's routing (None: the float64 first-argmax).  -> dict of truths (dh, dW, db, dw, reps, a), bounds (b_dh, b_dW, b_db, b_db_rounded,
    b_dw) and the near-tie count"""
    hidden, W, w, m, G = (np.asarray(a).astype(np.float64) for a in (hidden, W, w, m, G))
    bias = np.zeros(W.shape[0]) if bias is None else np.asarray(bias).astype(np.float64)
    B, T, H = hidden.shape
    V = W.shape[0]
    aW = np.abs(W)
    M = max(1, int((m != 0).sum()))
    r = dict(dh=np.zeros((B, T, H)), b_dh=np.zeros((B, T, H)), dW=np.zeros((V, H)), db=np.zeros(V), dw=np.zeros((B, T)), b_dw=np.zeros((B, T)),
             reps=np.zeros((B, V)), a=np.zeros((B, V), np.int64), ties=0, near=0)
    e_dW, s_dW, e_db, er_db, s_db, sr_db = np.zeros((V, H)), np.zeros((V, H)), np.zeros(V), np.zeros(V), np.zeros(V), np.zeros(V)
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
        er = np.where(live, b_dx + np.maximum(U16 * np.abs(dx), SUB16), 0.0)
        e = er if dx_fp16 else b_dx
        hb = hidden[b]
        r["dh"][b], r["b_dh"][b] = dx @ W, e @ aW + V * U32 * ((np.abs(dx) + e) @ aW)
        r["dW"] += dx.T @ hb
        e_dW += e.T @ np.abs(hb)
        s_dW += (np.abs(dx) + e).T @ np.abs(hb)
        r["db"] += dx.sum(0)
        e_db += b_dx.sum(0)
        s_db += np.abs(dx).sum(0)
        er_db += er.sum(0)
        sr_db += (np.abs(dx) + er).sum(0)
        r["dw"][b], r["b_dw"][b], r["reps"][b], r["a"][b] = dw[0], b_dw[0], reps[0], a[0]
    r["b_dW"] = e_dW + M * U32 * s_dW
    r["b_db"] = e_db + M * U32 * s_db
    r["b_db_rounded"] = er_db + M * U32 * sr_db
    return r


def random_case(B, T, V, H, seed):
    """-> hidden [B, T + 1, H] fp16, W fp16, bias fp32, w [B, T] fp32 (mixed signs), mask [B, T], G [B, V] fp32 (a tenth zeros)"""
    rng = np.random.default_rng(seed)
    hidden = rng.standard_normal((B, T + 1, H)).astype(np.float16)
    W = (rng.standard_normal((V, H)) * (2 / np.sqrt(H))).astype(np.float16)
    bias = (rng.standard_normal(V) * 0.1).astype(np.float32)
    w = rng.standard_normal((B, T)).astype(np.float32)
    lens = rng.integers(1, T + 1, B)
    lens[0] = T
    mask = (np.arange(T)[None] < lens[:, None]).astype(np.int64)
    mask[1, min(2, T - 1)] = 0                                                    # a masked token (between live ones where the length allows)
    mask[-1] = 0                                                                  # a fully masked passage
    G = (rng.standard_normal((B, V)) * (rng.random((B, V)) > 0.1)).astype(np.float32)
    return hidden, W, bias, w, mask, G


# ------------------------------------------------------------------------------------------ CPU part
def test_fixture_matches_float64_restatement():
    g = _golden()
    for name in CASES:
        hid, W, bias, w, mask = g[name + "_hidden"], g[name + "_W"], g[name + "_bias"], g[name + "_w"], g[name + "_mask"][:, 1:]
        _exact_logits(hid, W, bias)
        t = truth64(hid[:, 1:], W, bias, w, mask, g[name + "_G"], dx_fp16=False)
        assert t["near"] == 0, name                                               # the goldens hold no near-tie
        assert np.all(np.abs(g[name + "_reps"] - t["reps"]) <= 1e-5 * np.abs(t["reps"]) + 1e-30), name
        rows = g[name + "_dW_rows"]
        assert_within(g[name + "_dhidden"][:, 1:], t["dh"], t["b_dh"], name + " dhidden (fixture)")
        assert_within(g[name + "_dW"], t["dW"][rows], t["b_dW"][rows], name + " dW (fixture)")
        assert_within(g[name + "_dbias"], t["db"], t["b_db"], name + " dbias (fixture)")
        assert_within(g[name + "_dw"], t["dw"], t["b_dw"], name + " dL/dw (fixture)")
        assert not g[name + "_dhidden"][:, 0].any() and not g[name + "_dhidden"][:, 1:][mask == 0].any() and not g[name + "_dw"][mask == 0].any()
        G = g[name + "_G"]
        assert (G == 0).any() and (G < 0).any() and (G > 0).any() and g[name + "_dhidden"].any() and g[name + "_dW"].any()
    # the cases cover what they were designed for
    sm, rows = g["small_mask"], g["prod_dW_rows"]
    assert (sm[3, 1:] == 0).all() and sm[4, 1] == 1 and (sm[4, 3:] == 0).all() and sm[1, 3] == 0 and sm[1, 4] == 1
    assert np.array_equal(g["small_hidden"][1, 4], g["small_hidden"][1, 2]) and g["small_w"][1, 3] == g["small_w"][1, 1]    # the token tie
    a = truth64(g["small_hidden"][:, 1:], g["small_W"], g["small_bias"], g["small_w"], sm[:, 1:], g["small_G"])["a"]
    assert (a[1] != 3).all() and (a[1] == 1).any()                                # ... whose first token takes the route
    assert (g["neg_w"] < 0).all() and (g["neg_mask"][2, 1:] == 0).all() and g["neg_hidden"].shape[2] == 72
    assert g["prod_W"].shape == (30522, 16) and len(rows) >= 2048 and {0, 255, 256}.issubset(rows.tolist())
    assert set(range(30522 - 64, 30522)).issubset(rows.tolist()) and os.path.getsize(GOLDEN) < 1 << 20


def test_new_symbols_are_declared_mapped_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "dhr_hip.h")).read()
    vmap = open(os.path.join(ROOT, "dhr_amd", "csrc", "libdhr.map")).read()
    globs = re.findall(r"^\s*([a-z_*]+);", vmap.split("local:")[0], re.M)
    lib = _lib.load()
    for name in NEW:
        assert name + "(" in header and name in _lib.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
        assert any(fnmatch.fnmatch(name, p) for p in globs), globs
    assert lib.dhr_version() == 105
    from dhr_amd import _build
    assert "lexical_proj_train.hip" in _build.SOURCES and "lexical_proj_common.h" in _build.HEADERS
    from dhr_amd import lexical_proj_train as LPT
    assert callable(LPT.lexical_reps)


def test_workspace_obeys_its_bound():
    lib = _lib.load()
    for B, T, V, H in ((1, 1, 8, 8), (5, 70, 30522, 768), (128, 127, 30522, 768), (192, 149, 30522, 768), (128, 31, 30522, 1024), (16, 64, 30522, 1024),
                       (4096, 1, 202, 24), (3, 600, 762, 72), (2, 9, 202, 24), (8, 32, 30522, 1024)):
        n = lib.dhr_lexical_proj_train_workspace(B, T, V, H)
        assert 0 < n <= _ws_bound(B, T, H), (B, T, V, H, n)
    for bad in ((-1, 4, 8, 8), (1 << 30, 4, 8, 8), (2, 0, 8, 8), (2, 32768, 8, 8), (2, 4, 0, 8), (2, 4, 8, 0), (2, 4, 8, 12), (2, 4, 8, 1032)):
        assert lib.dhr_lexical_proj_train_workspace(*bad) == 0, bad


def _train(lib, **kw):
    """dhr_lexical_proj_train on made-up addresses: every bad argument must be refused before anything touches them."""
    a = dict(device=0, mem_kind=_lib.MEM_DEVICE, hidden=4096, value_dtype=_lib.VAL_F16, batch=2, n_tokens=3, skip=1, hidden_dim=16, ld_batch=64,
             ld_token=16, weight=4096, vocab=32, ld_weight=16, bias=4096, bias_dtype=_lib.VAL_F32, w=4096, ld_w=3, m=4096, ld_m=3, reps=4096,
             ld_reps=32, tok=4096, ld_tok=32, pwin=4096, ld_pwin=32, ws=4096, ws_bytes=1 << 20, stream=None)
    a.update(kw)
    return lib.dhr_lexical_proj_train(*a.values())


def _bwd(lib, **kw):
    a = dict(device=0, mem_kind=_lib.MEM_DEVICE, hidden=4096, value_dtype=_lib.VAL_F16, batch=2, n_tokens=3, skip=1, hidden_dim=16, ld_batch=64,
             ld_token=16, weight=4096, vocab=32, ld_weight=16, bias=4096, bias_dtype=_lib.VAL_F32, w=4096, ld_w=3, m=4096, ld_m=3, g=4096, ld_g=32,
             tok=4096, ld_tok=32, pwin=4096, ld_pwin=32, ws=4096, ws_bytes=1 << 20, gh=4096, gh_dtype=_lib.VAL_F16, ld_gh_batch=64, ld_gh_token=16,
             gw=4096, gw_dtype=_lib.VAL_F16, ld_gw=16, gb=4096, gb_dtype=_lib.VAL_F32, gtw=4096, ld_gtw=3, stream=None)
    a.update(kw)
    return lib.dhr_lexical_proj_backward(*a.values())


def test_bad_arguments_and_a_missing_device_are_statuses():
    import torch
    lib = _lib.load()
    common = [dict(hidden=None), dict(weight=None), dict(w=None), dict(m=None), dict(mem_kind=7), dict(value_dtype=5), dict(bias_dtype=5),
              dict(batch=-1), dict(n_tokens=0), dict(n_tokens=-2), dict(skip=-1), dict(skip=40000), dict(skip=2), dict(vocab=0), dict(hidden_dim=0),
              dict(hidden_dim=12, ld_token=12, ld_weight=12), dict(ld_token=15), dict(ld_batch=63), dict(ld_weight=8), dict(ld_w=2), dict(ld_m=2),
              dict(ld_tok=31), dict(ld_pwin=31), dict(tok=None), dict(pwin=None), dict(ws=None), dict(ws_bytes=64), dict(ws_bytes=-1), dict(ws=4100)]
    for b in common + [dict(reps=None), dict(ld_reps=31)]:
        assert _train(lib, **b) == _lib.ERR_INVALID, b
    for b in common + [dict(g=None), dict(ld_g=31), dict(gh_dtype=5), dict(gw_dtype=5), dict(gb_dtype=5), dict(ld_gh_token=15), dict(ld_gh_batch=63),
                       dict(ld_gw=8), dict(ld_gtw=2)]:
        assert _bwd(lib, **b) == _lib.ERR_INVALID, b
    for call in (_train, _bwd):
        assert call(lib, hidden_dim=12, ld_token=12, ld_weight=12) == _lib.ERR_INVALID and b"multiple of 8" in lib.dhr_last_error()
        assert call(lib, ws_bytes=64) == _lib.ERR_INVALID and b"workspace" in lib.dhr_last_error()
        assert call(lib, value_dtype=_lib.VAL_F32) == _lib.ERR_UNSUPPORTED                     # fp32 operands are rounded by the caller
        wide = dict(ld_gh_token=1032, ld_gh_batch=4128, ld_gw=1032) if call is _bwd else {}
        assert call(lib, hidden_dim=1032, ld_token=1032, ld_batch=4128, ld_weight=1032, **wide) == _lib.ERR_UNSUPPORTED     # H above 1024
        long = dict(ld_gh_batch=1 << 20, ld_gtw=32768) if call is _bwd else {}
        assert call(lib, n_tokens=32768, ld_batch=1 << 20, ld_w=32768, ld_m=32768, **long) == _lib.ERR_UNSUPPORTED         # tok is int16
        assert call(lib, mem_kind=_lib.MEM_HOST) == _lib.ERR_UNSUPPORTED and b"live on the device" in lib.dhr_last_error()
        assert call(lib, batch=0) == _lib.DHR_OK                                               # nothing to do: no device is touched
        assert call(lib, bias=None, bias_dtype=99, batch=0) == _lib.DHR_OK                     # no bias: its dtype is not looked at
    assert _bwd(lib, gh=None, gw=None, gb=None, gtw=None, ws=None) == _lib.DHR_OK              # no gradient wanted: nothing is launched
    assert _bwd(lib, gh=None, gw=None, gb=None, gtw=None, gh_dtype=99, gw_dtype=99, gb_dtype=99) == _lib.DHR_OK
    if not torch.cuda.is_available():                                                          # valid calls without a device: a status
        assert _train(lib) == _lib.ERR_HIP and _bwd(lib) == _lib.ERR_HIP


def test_wrapper_raises_before_touching_the_library(monkeypatch):
    import torch
    from dhr_amd import lexical_proj_train as LPT

    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", no_library)
    h, W, b = torch.zeros((2, 5, 16), dtype=torch.float16), torch.zeros((32, 16), dtype=torch.float16), torch.zeros((32,))
    w, m = torch.ones((2, 4)), torch.ones((2, 4), dtype=torch.long)
    for args in ((h[0], W, b, w, m, 1), (h[None], W, b, w, m, 1), (h, W[0], b, w, m, 1), (h, W[:, :8], b, w, m, 1), (h, W, b[:8], w, m, 1),
                 (h, W, b[None], w, m, 1), (h, W, b, w, m, 0), (h, W, b, w[:, :3], m, 1), (h, W, b, w, m[:, :3], 1), (h, W, b, w[..., None, None], m, 1),
                 (h, W, b, w, m, 5), (h, W, b, w, m, 7), (h, W, b, w, m, -1), (h[:, :0], W, b, w[:, :0], m[:, :0], 0), (h, W[:0], b[:0], w, m, 1)):
        with pytest.raises(ValueError):
            LPT.lexical_reps(*args)
    with pytest.raises(ValueError, match="no tokens"):
        LPT.lexical_reps(h, W, b, w, m, skip_tokens=5)
    for args in ((h.double(), W, b, w, m, 1), (h, W.to(torch.bfloat16), b, w, m, 1), (h, W, b.double(), w, m, 1), (h, W, b, w.long(), m, 1),
                 (h[..., :12], W[:, :12], b, w, m, 1), (h.numpy(), W.numpy(), b.numpy(), w.numpy(), m.numpy(), 1), (h, W, b.numpy(), w, m, 1)):
        with pytest.raises(_lib.DhrError):
            LPT.lexical_reps(*args)
    with pytest.raises(_lib.DhrError, match="GPU"):                               # CPU tensors: there is no CPU implementation
        LPT.lexical_reps(h, W, b, w, m, skip_tokens=1)
    with pytest.raises(_lib.DhrError, match="GPU"):
        LPT.lexical_reps(h.float(), W.float(), None, w[..., None], m[..., None], skip_tokens=1, return_tokens=True)


def test_seeds_keep_the_truth_inside_the_near_tie_cap():
    for B, T, V, H, seed in RANDOM:
        hidden, W, bias, w, mask, G = random_case(B, T, V, H, seed)
        for bb in (bias, None):
            x = hidden[:, 1:].astype(np.float64) @ W.astype(np.float64).T + (0 if bb is None else bb.astype(np.float64))
            near = forward64(x, w, mask)[4]
            assert near.sum() <= 1e-4 * B * V, (B, T, V, H, seed, int(near.sum()))
        assert (mask[-1] == 0).all() and (mask[0] == 1).all() and (w < 0).any() and (w > 0).any()


# ------------------------------------------------------------------------------------------ GPU part
def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _np(t):
    return t.detach().float().cpu().numpy()


def _bits(t):
    import torch
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _run(hidden, W, bias, w, mask, G, skip=1, dtype=None, view=False, need=(True, True, True, True)):
    """One forward + backward of the library on numpy operands.  hidden is the model's [B, L, H]; view: pass hidden[:, skip:] with
    skip_tokens=0.  -> (reps, tok, dhidden [B, L, H], dW, dbias, dw [B, T, 1]) torch tensors (None where not needed)"""
    import torch
    from dhr_amd import lexical_proj_train as LPT
    dtype = dtype or torch.float16
    h = _dev(hidden, dtype).requires_grad_(need[0])
    Wt = _dev(W, dtype).requires_grad_(need[1])
    bt = None if bias is None else _dev(bias).requires_grad_(need[2])
    wt = _dev(w)[..., None].requires_grad_(need[3])                                # [B, T, 1], as term_weight_trans returns it
    out, tok = LPT.lexical_reps(h[:, skip:] if view else h, Wt, bt, wt, _dev(mask), skip_tokens=0 if view else skip, return_tokens=True)
    assert out.dtype == torch.float32 and tok.dtype == torch.int16 and out.requires_grad and not tok.requires_grad
    out.backward(_dev(G))
    return out.detach(), tok, h.grad, Wt.grad, None if bt is None else bt.grad, wt.grad


def _check(tag, t, mask, dh, dW, db, dw, fp16, rows=None, db_bound="b_db"):
    """gradients (torch, dh of the tokens after the skipped ones) against truth64's result -> {name: worst error / bound}"""
    rows = slice(None) if rows is None else rows
    res = {"dhidden": assert_within(_np(dh), t["dh"], t["b_dh"], tag + " dhidden", fp16=fp16),
           "dW": assert_within(_np(dW)[rows], t["dW"][rows], t["b_dW"][rows], tag + " dW", fp16=fp16),
           "dL/dw": assert_within(_np(dw)[..., 0], t["dw"], t["b_dw"], tag + " dL/dw")}
    if db is not None:
        res["dbias"] = assert_within(_np(db), t["db"], t[db_bound], tag + " dbias", fp16=db.element_size() == 2)
    assert not _np(dh)[mask == 0].any() and not _np(dw)[..., 0][mask == 0].any(), tag
    return res


@pytest.mark.gpu
def test_goldens_on_gpu():
    import torch
    from dhr_amd import lexical_proj as LP
    from dhr_amd import lexical_train as LT
    g = _golden()
    for name in CASES:
        hid, W, bias, w, mask, G = (g[name + k] for k in ("_hidden", "_W", "_bias", "_w", "_mask", "_G"))
        mask = mask[:, 1:]
        _exact_logits(hid, W, bias)
        for dt in (torch.float16, torch.float32):
            out, tok, dh, dW, db, dw = _run(hid, W, bias, w, mask, G, dtype=dt)
            t = truth64(hid[:, 1:], W, bias, w, mask, G, tok=tok.cpu().numpy(), what=name)
            assert t["ties"] == 0 and np.array_equal(tok.cpu().numpy(), t["a"]), name
            enc = LP.lexical_reps(_dev(hid)[:, 1:], _dev(W), _dev(bias), _dev(w), _dev(mask))
            assert torch.equal(_bits(out), _bits(enc)), name                       # bit-equal to the encoding op
            logits = torch.nn.functional.linear(_dev(hid).float(), _dev(W).float(), _dev(bias))
            _, tok_lt = LT.lexical_reps(logits, _dev(w), _dev(mask), skip_tokens=1, return_tokens=True)
            assert torch.equal(tok, tok_lt), name                                  # masked winners are named as the head on logits names them
            assert dh.dtype == dt and dW.dtype == dt and db.dtype == torch.float32 and dh.shape == hid.shape and dw.shape == w.shape + (1,)
            assert not dh[:, 0].any()
            rows = g[name + "_dW_rows"]
            _check(f"{name} {dt}", t, mask, dh[:, 1:], dW, db, dw, dt == torch.float16)
            # ... and against what the reference's autograd returned, each within its bound of the truth
            f = truth64(hid[:, 1:], W, bias, w, mask, G, dx_fp16=False)
            r16 = lambda x: np.maximum(U16 * np.abs(x), SUB16) if dt == torch.float16 else 0                           # noqa: E731
            assert np.all(np.abs(_np(dh)[:, 1:] - g[name + "_dhidden"][:, 1:]) <= t["b_dh"] + f["b_dh"] + r16(g[name + "_dhidden"][:, 1:]))
            assert np.all(np.abs(_np(dW)[rows] - g[name + "_dW"]) <= (t["b_dW"] + f["b_dW"])[rows] + r16(g[name + "_dW"]))
            assert np.all(np.abs(_np(db) - g[name + "_dbias"]) <= t["b_db"] + f["b_db"])
            assert np.all(np.abs(_np(dw)[..., 0] - g[name + "_dw"]) <= 2 * t["b_dw"])


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,V,H,seed", RANDOM)
def test_random_cases_against_the_float64_truth(B, T, V, H, seed):
    import torch
    from dhr_amd import lexical_proj as LP
    hidden, W, bias, w, mask, G = random_case(B, T, V, H, seed)
    tag = f"random {B}x{T}x{V}x{H}"
    # fp16 operands with a bias: the whole tensor with skip_tokens=1 and the [:, 1:] view with skip_tokens=0, bit for bit
    whole = _run(hidden, W, bias, w, mask, G)
    view = _run(hidden, W, bias, w, mask, G, view=True)
    for x, y in zip(whole, view):
        assert torch.equal(_bits(x), _bits(y)), tag
    out, tok, dh, dW, db, dw = whole
    assert torch.equal(_bits(out), _bits(LP.lexical_reps(_dev(hidden)[:, 1:], _dev(W), _dev(bias), _dev(w), _dev(mask)))), tag
    t = truth64(hidden[:, 1:], W, bias, w, mask, G, tok=tok.cpu().numpy(), inexact=True, what=tag)
    assert t["ties"] <= 1e-4 * B * V, tag
    assert not dh[:, 0].any() and not dh[-1].any() and dh.dtype == torch.float16 and dW.dtype == torch.float16 and db.dtype == torch.float32
    res = _check(tag + " fp16", t, mask, dh[:, 1:], dW, db, dw, True)
    # fp32 operands (the same values: they round to fp16 exactly once) without a bias
    out32, tok32, dh32, dW32, db32, dw32 = _run(hidden, W, None, w, mask, G, dtype=torch.float32)
    assert db32 is None and dh32.dtype == torch.float32 and dW32.dtype == torch.float32
    t = truth64(hidden[:, 1:], W, None, w, mask, G, tok=tok32.cpu().numpy(), inexact=True, what=tag + " no bias")
    assert t["ties"] <= 1e-4 * B * V and not dh32[:, 0].any(), tag
    res32 = _check(tag + " fp32, no bias", t, mask, dh32[:, 1:], dW32, None, dw32, False)
    print(f"{tag}: worst error / bound fp16 {res}, fp32 {res32}")
    # a batch with every token masked: every gradient is an exact zero
    _, _, dh0, dW0, db0, dw0 = _run(hidden, W, bias, w, np.zeros_like(mask), G)
    assert not dh0.any() and not dW0.any() and not db0.any() and not dw0.any(), tag


@pytest.mark.gpu
def test_exact_operands_at_production_geometry():
    """B = 4, T = 127, V = 30522, H = 768 with the exact-arithmetic operands; the parent composition on the same device is held to the same
    bounds (its dbias to the bound of a sum of ROUNDED dx, see the module docstring)."""
    import torch
    from dhr_amd import lexical_train as LT
    B, T, V, H = 4, 127, 30522, 768
    rng = np.random.default_rng(41)
    hidden = (rng.integers(-8, 9, (B, T + 1, H)) / 4).astype(np.float16)
    W = (rng.choice(np.array([-1.0, 0.0, 0.0, 1.0]), (V, H)) / 8).astype(np.float16)
    bias = (rng.integers(-16, 17, V) / 32).astype(np.float32)
    w = rng.standard_normal((B, T)).astype(np.float16).astype(np.float32)
    lens = np.array([T, 37, 90, 64])
    mask = (np.arange(T)[None] < lens[:, None]).astype(np.int64)
    mask[2, 10] = 0
    G = (rng.standard_normal((B, V)) * (rng.random((B, V)) > 0.1)).astype(np.float32)
    x = hidden[0, 1:].astype(np.float64) @ W.astype(np.float64).T + bias
    assert np.array_equal(x.astype(np.float16).astype(np.float64), x) and np.abs(x).max() < 2 ** 9
    out, tok, dh, dW, db, dw = _run(hidden, W, bias.astype(np.float16), w, mask, G)
    t = truth64(hidden[:, 1:], W, bias, w, mask, G, tok=tok.cpu().numpy(), what="production")
    assert t["ties"] <= 1e-4 * B * V and not dh[:, 0].any() and db.dtype == torch.float16
    res = _check("production", t, mask, dh[:, 1:], dW, db, dw, True)
    # the parent composition: F.linear in fp16, the head on logits, autograd
    h = _dev(hidden).requires_grad_(True)
    Wt, bt, wt = _dev(W).requires_grad_(True), _dev(bias, torch.float16).requires_grad_(True), _dev(w)[..., None].requires_grad_(True)
    p_out, p_tok = LT.lexical_reps(torch.nn.functional.linear(h, Wt, bt), wt, _dev(mask), skip_tokens=1, return_tokens=True)
    p_out.backward(_dev(G))
    assert torch.allclose(p_out.detach(), out, rtol=1e-5, atol=1e-30)              # exact logits: the two forwards differ by fp32 roundings only
    tp = truth64(hidden[:, 1:], W, bias, w, mask, G, tok=p_tok.cpu().numpy(), what="production, parent")
    res_p = _check("production, parent", tp, mask, h.grad[:, 1:], Wt.grad, bt.grad, wt.grad, True, db_bound="b_db_rounded")
    print(f"production geometry: worst error / bound {res}; parent composition {res_p}")


@pytest.mark.gpu
def test_bit_identity_and_gradient_subsets():
    import torch
    B, T, V, H, seed = 6, 50, 1030, 136, 21
    hidden, W, bias, w, mask, G = random_case(B, T, V, H, seed)
    runs = [_run(hidden, W, bias, w, mask, G) for _ in range(2)]
    for x, y in zip(*runs):
        assert torch.equal(_bits(x), _bits(y))
    _, _, dh, dW, db, dw = runs[0]
    for need in ((True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True),
                 (True, False, False, True), (False, True, True, False)):
        got = _run(hidden, W, bias, w, mask, G, need=need)[2:]
        for wanted, x, ref in zip(need, got, (dh, dW, db, dw)):
            assert (x is not None) == wanted and (x is None or torch.equal(_bits(x), _bits(ref))), need
    # twice through one graph
    from dhr_amd import lexical_proj_train as LPT
    h, Wt = _dev(hidden).requires_grad_(True), _dev(W).requires_grad_(True)
    out = LPT.lexical_reps(h, Wt, _dev(bias), _dev(w), _dev(mask), skip_tokens=1)
    out.backward(_dev(G), retain_graph=True)
    h.grad = Wt.grad = None
    out.backward(_dev(G))
    assert torch.equal(_bits(h.grad), _bits(dh)) and torch.equal(_bits(Wt.grad), _bits(dW))


@pytest.mark.gpu
def test_composed_training_step():
    """hidden states -> lexical reps of queries and passages -> listwise_gip_scores -> cross-entropy -> backward, with this op and with the
    parent composition (F.linear in fp16, the head on logits), on exact-arithmetic operands: the parent's fp16 logits are then the exact
    logits too, and both steps answer to the same float64 truth without any widening.  The upstream dL/dreps of the two steps differ by the
    fp32 roundings of their reps, so the gradients of each step -- the parent's as well -- are held to the bounds of the truth under ITS OWN
    dL/dreps and routing (tests/test_lexical_train.py does the same); the parent's dbias to the bound of a sum of ROUNDED dx (the module
    docstring).  The reps of both steps are held to the truth's: every candidate (p * w) * m carries a relative error of at most
    (kappa + 2) u with kappa <= 8 + 2 max(d) + 2 s of tests/test_lexical_train.py, and with w >= 0 the largest candidate is the truth itself."""
    import torch
    from dhr_amd import gip_scores as GS
    from dhr_amd import lexical_proj_train as LPT
    from dhr_amd import lexical_train as LT
    V, H, dims, remove, n_q, n_pass = 4026, 72, 64, 58, 3, 2
    rng = np.random.default_rng(29)
    W = (rng.choice(np.array([-1.0, 0.0, 0.0, 1.0]), (V, H)) / 8).astype(np.float16)
    bias = (rng.integers(-16, 17, V) / 32).astype(np.float32)
    sides = {}
    for side, B, L in (("q", n_q, 8), ("p", n_q * n_pass, 12)):
        hid = (rng.integers(-8, 9, (B, L, H)) / 4).astype(np.float16)
        w = np.abs(rng.standard_normal((B, L - 1))).astype(np.float16).astype(np.float32)
        mask = (np.arange(L - 1)[None] < rng.integers(2, L, (B, 1))).astype(np.int64)
        sides[side] = (hid, w, mask, _exact_logits(hid[:, 1:], W, bias))

    def step(head):
        leaves, res = {}, {}
        for side, (hid, w, mask, _) in sides.items():
            h, Wt, bt = _dev(hid).requires_grad_(True), _dev(W).requires_grad_(True), _dev(bias, torch.float16).requires_grad_(True)
            wt = _dev(w)[..., None].requires_grad_(True)
            reps, tok = head(h, Wt, bt, wt, _dev(mask))
            reps.retain_grad()
            leaves[side], res[side] = (h, Wt, bt, wt), (reps, tok)
        scores = GS.listwise_gip_scores(res["q"][0], res["p"][0], n_q, dims, remove)
        loss = torch.nn.functional.cross_entropy(scores, torch.arange(n_q, device="cuda") * n_pass)
        loss.backward()
        return float(loss.detach()), {s: (res[s][0].detach(), res[s][0].grad, res[s][1]) + tuple(x.grad for x in leaves[s]) for s in sides}

    loss_new, new = step(lambda h, Wt, bt, wt, m: LPT.lexical_reps(h, Wt, bt, wt, m, skip_tokens=1, return_tokens=True))
    loss_old, old = step(lambda h, Wt, bt, wt, m: LT.lexical_reps(torch.nn.functional.linear(h, Wt, bt), wt, m, skip_tokens=1, return_tokens=True))
    print(f"composed step: loss {loss_new:.7f} (this op) / {loss_old:.7f} (parent composition)")
    for side, (hid, w, mask, x) in sides.items():
        kappa = 8 + 2 * (x.max(-1) - x.min(-1)).max() + 2 * (-(-V // 1024) + 10)
        for which, got, db_bound in (("this op", new, "b_db"), ("parent", old, "b_db_rounded")):
            reps, G, tok, dh, dW, db, dw = got[side]
            tag = f"composed {side}, {which}"
            assert G.any() and not dh[:, 0].any(), tag
            t = truth64(hid[:, 1:], W, bias, w, mask, _np(G), tok=tok.cpu().numpy(), what=tag)
            assert np.all(np.abs(_np(reps) - t["reps"]) <= (kappa + 2) * U32 * t["reps"]), tag
            res = _check(tag, t, mask, dh[:, 1:], dW, db, dw, True, db_bound=db_bound)
            print(f"{tag}: worst error / bound {res}")


@pytest.mark.gpu
def test_backward_reads_the_tensors_that_saved_tensor_hooks_return():
    """Under torch.autograd.graph.save_on_cpu the saved tensors leave the device after the forward and come back at new addresses; the
    fp16 copies of fp32 operands, the fp32 term weights and mask, tok, pwin and the workspace are freed in between, and the test hands their
    memory to other tensors (zeros: an empty token list to whoever reads a stale workspace).  The gradients are bit-identical to those of a plain run."""
    import torch
    from dhr_amd import lexical_proj_train as LPT
    B, T, V, H, seed = 5, 70, 762, 72, 11
    hidden, W, bias, w, mask, G = random_case(B, T, V, H, seed)
    plain = _run(hidden, W, bias, w, mask, G, dtype=torch.float32)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    h, Wt, bt = (_dev(a, torch.float32).requires_grad_(True) for a in (hidden, W, bias))
    wt = _dev(w)[..., None].requires_grad_(True)
    with torch.autograd.graph.save_on_cpu():
        out, tok = LPT.lexical_reps(h, Wt, bt, wt, _dev(mask), skip_tokens=1, return_tokens=True)
    tok = tok.clone()
    torch.cuda.synchronize()
    junk = [torch.zeros((n,), dtype=torch.float16, device="cuda") for n in (B * (T + 1) * H, V * H, 2 * B * T, 2 * B * T, 2 * B * V)
            for _ in range(2)]
    torch.cuda.synchronize()
    out.backward(_dev(G))
    got = (out.detach(), tok, h.grad, Wt.grad, bt.grad, wt.grad)
    for x, y in zip(plain, got):
        assert torch.equal(_bits(x), _bits(y))
    del junk


@pytest.mark.gpu
def test_memory_has_no_btv_term():
    """Peak device memory over a forward plus backward, everything but the inputs counted, at T = 127, V = 30522, H = 768 (fp16): at B = 128
    it stays under the fp16 logits alone, and from B = 64 to B = 128 it grows by at most 64 * (16 V + 8 T H + 512 T) bytes -- reps, tok, pwin
    and one fp32 copy of g; dhidden in two dtypes; per-token state: there is no room for a B * T * V term in that."""
    import torch
    from dhr_amd import lexical_proj_train as LPT
    T, V, H = 127, 30522, 768
    gen = torch.Generator(device="cuda").manual_seed(31)
    W = (torch.randn((V, H), generator=gen, device="cuda") * 0.07).half().requires_grad_(True)
    bias = (torch.randn((V,), generator=gen, device="cuda") * 0.1).requires_grad_(True)
    peaks = {}
    for B in (64, 128, 64, 128):                                                   # (the first round loads the library and warms the allocator)
        hidden = torch.randn((B, T + 1, H), generator=gen, device="cuda").half().requires_grad_(True)
        w = torch.randn((B, T, 1), generator=gen, device="cuda").half().requires_grad_(True)
        mask = torch.ones((B, T), dtype=torch.int64, device="cuda")
        G = torch.randn((B, V), generator=gen, device="cuda")
        W.grad = bias.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        LPT.lexical_reps(hidden, W, bias, w, mask, skip_tokens=1).backward(G)
        torch.cuda.synchronize()
        peaks[B] = torch.cuda.max_memory_allocated() - before
        del hidden, w, mask, G
    logits = 2 * 128 * T * V
    growth, cap = peaks[128] - peaks[64], 64 * (16 * V + 8 * T * H + 512 * T)
    print(f"memory: peak over the inputs {peaks[64] / 1e6:.1f} MB at B = 64, {peaks[128] / 1e6:.1f} MB at B = 128 (the fp16 logits alone: "
          f"{logits / 1e6:.1f} MB); growth {growth / 1e6:.1f} MB, cap {cap / 1e6:.1f} MB")
    assert peaks[128] < logits
    assert growth <= cap


@pytest.mark.gpu
def test_timing_printout():
    """Forward + backward against the parent composition (F.linear in fp16, lexical_train.lexical_reps, .backward()) at B = 128, L = 128,
    H = 768, V = 30522, every token unmasked: device events, 3 warm-ups, median of 10.  A printout, not a threshold."""
    import torch
    from dhr_amd import lexical_proj_train as LPT
    from dhr_amd import lexical_train as LT
    B, L, V, H = 128, 128, 30522, 768
    hidden = torch.randn((B, L, H), device="cuda").half().requires_grad_(True)
    W = (torch.randn((V, H), device="cuda") * 0.07).half().requires_grad_(True)
    bias = (torch.randn((V,), device="cuda") * 0.1).half().requires_grad_(True)
    w = torch.randn((B, L - 1, 1), device="cuda").half().requires_grad_(True)
    mask = torch.ones((B, L - 1), dtype=torch.int64, device="cuda")
    G = torch.randn((B, V), device="cuda")

    def fused():
        LPT.lexical_reps(hidden, W, bias, w, mask, skip_tokens=1).backward(G)

    def parent():
        LT.lexical_reps(torch.nn.functional.linear(hidden, W, bias), w, mask, skip_tokens=1).backward(G)

    res = {}
    for name, fn in (("fused", fused), ("parent", parent)):
        times = []
        for it in range(13):
            hidden.grad = W.grad = bias.grad = w.grad = None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= 3:
                times.append(e0.elapsed_time(e1))
        res[name] = float(np.median(times))
        torch.cuda.empty_cache()
    print(f"lexical projection head fwd+bwd B={B} L={L} H={H} V={V} fp16: fused {res['fused']:.2f} ms, linear + head on logits {res['parent']:.2f} ms, "
          f"{res['parent'] / res['fused']:.2f}x")
