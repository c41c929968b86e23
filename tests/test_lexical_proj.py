"""The lexical head with the vocabulary projection fused in (dhr_amd/lexical_proj.py, dhr_amd/csrc/lexical_proj.hip) against the reference's
own encoder code (tests/golden/lexical_proj_golden.npz, made by tests/golden/make_golden_lexical_proj.py), a float64 truth, and the parent
path (torch projection + dhr_amd.lexical) on the same device.

Operands.  The goldens and the production-geometry test use EXACT-ARITHMETIC operands (hidden = randint(-8..8)/4, W = choice(-1,0,0,1)/8,
bias = randint(-16..16)/32): every partial sum of a logit is a multiple of 2^-5 below 2^9, so fp32 accumulation in any order is exact and the
logits are fp16 values.  The tests assert that of the truth before they look at the kernel.  On them the tolerance rule of
test_lexical_head.py holds unchanged (fp32 within 1e-5 |ref| + 1e-30; fp16 bit-equal up to counted midpoint exemptions; indices equal up to
counted near-ties; zero exemptions on the goldens; signs of zero bit for bit).

Inexact operands.  The kernel's logit differs from the float64 one by the fp32 accumulation error, at most (H + 1) 2^-24 (sum_k |h||W| +
|bias|) in any order, and the normaliser by as much again relatively; with A[b][t] = max_v (sum_k |h||W| + |bias|) a contribution
c[b][t][v] = p w mask is off by at most |c| (2 (H + 2) 2^-24 A[b][t] + 1e-5), the second term being the head's own tolerance.  A maximum
moves by no more than the largest move of its candidates, so  tol[b][v] = max_t |c[b][t][v]| (2 (H + 2) 2^-24 A[b][t] + 1e-5)  bounds the
reps, and the maximum of tol over the groups of a slice bounds a densified value.  At H = 72 the bound is sharp enough that logits rounded
to fp16 break it; at H = 768 it pins tiling and tails.

CPU part: fixture vs float64 restatement, symbols, workspace bound, statuses.  GPU part: -m gpu."""
import fnmatch
import os
import re

import numpy as np
import pytest

from dhr_amd import _lib
from dhr_amd import lexical as LX
from tests.test_lexical_head import (aggregate_f64, check_f32, check_zero_signs, contributions_f64, densify_f64, fp16_exemptions,
                                     index_exemptions, reps_f64, _first_max)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lexical_proj_golden.npz")
CASES = ("prod", "small", "neg", "pad")
NEW = ("dhr_lexical_proj_workspace", "dhr_lexical_proj_head")


def _golden():
    return np.load(GOLDEN)


def _bound(B, T, V):
    return 4 * B * V + 256 * B * T + 65536


def _exact_logits(hidden, W, bias):
    """float64 logits of exact-arithmetic operands, after asserting the recipe's promise: the fp32 product in another order is the same
    number, and it is an fp16 value."""
    h, w = hidden.astype(np.float64), W.astype(np.float64)
    x = h @ w.T + (0 if bias is None else bias.astype(np.float64))
    x32 = hidden.astype(np.float32) @ W.astype(np.float32).T + (0 if bias is None else bias.astype(np.float32))
    assert np.array_equal(x32.astype(np.float64), x)
    assert np.array_equal(x.astype(np.float16).astype(np.float64), x)
    assert np.abs(x).max() < 2 ** 9
    return x


# ------------------------------------------------------------------------------------------ CPU part
def test_fixture_matches_float64_restatement():
    g = _golden()
    seen_tie = False
    for name in CASES:
        x = _exact_logits(g[name + "_hidden"], g[name + "_W"], g[name + "_bias"])
        w, m = g[name + "_w"], g[name + "_mask"][:, 1:]
        ref, zero = reps_f64(x[:, 1:], w, m)
        rep = g[name + "_reps"]
        check_f32(rep, ref, name)
        check_zero_signs(rep, ref, zero, name)
        dims, remove, agg = (int(v) for v in g[name + "_geom"])
        if dims:                                          # the epilogues are selections: exact on the reference's own reps
            v, i = densify_f64(rep.astype(np.float64), dims, remove)
            assert np.array_equal(v.astype(np.float32).view(np.uint32), g[name + "_dval"].view(np.uint32))
            assert np.array_equal(i, g[name + "_didx"])
            grp = rep[:, remove:].reshape(rep.shape[0], -1, dims)
            seen_tie |= bool(((grp == grp.max(1, keepdims=True)).sum(1) > 1)[grp.max(1) > 0].any())
        for full, tag in ((True, "_afull"), (False, "_asemi")):
            a = aggregate_f64(rep.astype(np.float64), agg, full).astype(np.float32)
            assert np.array_equal(a.view(np.uint32), g[name + tag].view(np.uint32)), (name, tag)
    # the cases cover what the issue lists: a fully masked passage, one masked from the middle, a masked token between unmasked ones,
    # all-negative term weights, a group tie
    sm = g["small_mask"]
    assert (sm[3, 1:] == 0).all() and sm[4, 1] == 1 and (sm[4, 3:] == 0).all() and sm[1, 3] == 0 and sm[1, 4] == 1
    assert (g["neg_w"] < 0).all() and (g["neg_mask"][2, 1:] == 0).all() and seen_tie
    assert g["prod_W"].shape == (30522, 16) and g["neg_hidden"].shape[2] == 72 and os.path.getsize(GOLDEN) < 1 << 20


def test_new_symbols_are_declared_mapped_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "dhr_hip.h")).read()
    vmap = open(os.path.join(ROOT, "dhr_amd", "csrc", "libdhr.map")).read()
    globs = re.findall(r"^\s*([a-z_*]+);", vmap.split("local:")[0], re.M)
    lib = _lib.load()
    for name in NEW:
        assert name + "(" in header and name in _lib.EXPORTS and hasattr(lib, name)
        assert any(fnmatch.fnmatch(name, p) for p in globs), globs
    assert lib.dhr_version() == 105
    from dhr_amd import _build
    assert "lexical_proj.hip" in _build.SOURCES
    from dhr_amd import lexical_proj as LP
    for fn in ("lexical_reps", "densify_lexical_into", "aggregate_lexical_into"):
        assert callable(getattr(LP, fn))


def test_workspace_obeys_its_bound():
    lib = _lib.load()
    for B, T, V in ((1, 1, 8), (5, 70, 30522), (128, 127, 30522), (128, 31, 30522), (16, 64, 30522), (4096, 1, 202), (3, 600, 762)):
        sizes = [lib.dhr_lexical_proj_workspace(B, T, V, mode) for mode in (_lib.LEX_RAW, _lib.LEX_DENSIFY, _lib.LEX_AGG_FULL, _lib.LEX_AGG_SEMI)]
        assert all(0 < s <= _bound(B, T, V) for s in sizes), (B, T, V, sizes)
        assert sizes[0] <= sizes[1] - 4 * B * V + 256 and sizes[1] == sizes[2] == sizes[3]     # raw reps are the output itself
    assert lib.dhr_lexical_proj_workspace(-1, 4, 8, 0) == 0 and lib.dhr_lexical_proj_workspace(1 << 30, 4, 8, 0) == 0


def _call(lib, **kw):
    """dhr_lexical_proj_head on made-up addresses: every bad argument must be refused before anything touches them."""
    a = dict(device=0, mem_kind=_lib.MEM_DEVICE, mode=_lib.LEX_DENSIFY, hidden=4096, value_dtype=_lib.VAL_F16, batch=2, n_tokens=3, hidden_dim=16,
             ld_batch=48, ld_token=16, weight=4096, vocab=32, ld_weight=16, bias=4096, bias_dtype=_lib.VAL_F32, w=4096, ld_w=3, m=4096, ld_m=3,
             dims=8, remove=0, val=4096, val_dtype=_lib.VAL_F16, ld_val=8, idx=4096, idx_dtype=_lib.IDX_U8, ld_idx=8, cls=None,
             cls_dtype=_lib.VAL_F16, ld_cls=0, cls_dim=0, ws=4096, ws_bytes=1 << 20, stream=None)
    a.update(kw)
    return lib.dhr_lexical_proj_head(*a.values())


def test_bad_arguments_and_a_missing_device_are_statuses():
    import torch
    lib = _lib.load()
    bad = [dict(hidden=None), dict(weight=None), dict(w=None), dict(m=None), dict(val=None), dict(mem_kind=_lib.MEM_HOST), dict(mem_kind=7),
           dict(mode=9), dict(value_dtype=5), dict(bias_dtype=5), dict(val_dtype=5), dict(batch=-1), dict(n_tokens=0), dict(vocab=0),
           dict(hidden_dim=0), dict(hidden_dim=12, ld_token=12, ld_weight=12), dict(ld_token=15), dict(ld_batch=40), dict(ld_weight=8),
           dict(ld_w=2), dict(ld_m=2), dict(dims=7), dict(dims=0), dict(remove=-2), dict(ld_val=7), dict(idx=None), dict(idx_dtype=_lib.IDX_I8),
           dict(ld_idx=4), dict(cls_dim=4), dict(ws=None), dict(ws_bytes=64), dict(ws_bytes=-1), dict(ws=4100)]
    for b in bad:
        assert _call(lib, **b) == _lib.ERR_INVALID, b
    assert _call(lib, dims=7) == _lib.ERR_INVALID and b"densified" in lib.dhr_last_error()
    assert _call(lib, hidden_dim=12, ld_token=12, ld_weight=12) == _lib.ERR_INVALID and b"multiple of 8" in lib.dhr_last_error()
    assert _call(lib, ws_bytes=64) == _lib.ERR_INVALID and b"workspace" in lib.dhr_last_error()
    assert _call(lib, value_dtype=_lib.VAL_F32) == _lib.ERR_UNSUPPORTED                    # fp32 operands are not built
    assert _call(lib, mode=_lib.LEX_RAW, ld_val=32) == _lib.ERR_UNSUPPORTED                # raw reps are fp32
    assert _call(lib, batch=0) == _lib.DHR_OK
    assert _call(lib, bias=None, bias_dtype=99, batch=0) == _lib.DHR_OK                    # no bias: its dtype is not looked at
    from dhr_amd import lexical_proj as LP
    h, W = torch.zeros((2, 3, 16), dtype=torch.float16), torch.zeros((32, 16), dtype=torch.float16)
    w, m = torch.ones((2, 3)), torch.ones((2, 3))
    with pytest.raises(_lib.DhrError, match="GPU"):
        LP.lexical_reps(h, W, None, w, m)
    with pytest.raises(_lib.DhrError, match="GPU"):
        LP.lexical_reps(h.numpy(), W.numpy(), None, w.numpy(), m.numpy())
    with pytest.raises(_lib.DhrError, match="GPU"):
        LP.densify_lexical_into(h, W, None, w, m, torch.zeros((2, 8), dtype=torch.float16), torch.zeros((2, 8), dtype=torch.uint8), 8, 0)
    with pytest.raises(ValueError, match="cannot be densified"):                           # the geometry checks and texts of lexical.py
        LP.densify_lexical_into(h, W, None, w, m, torch.zeros((2, 7), dtype=torch.float16), torch.zeros((2, 7), dtype=torch.uint8), 7, 1)
    with pytest.raises(RuntimeError, match="is invalid for input of size"):
        LP.aggregate_lexical_into(h, torch.zeros((1000, 16), dtype=torch.float16), None, w, m, torch.zeros((2, 8), dtype=torch.float16), 8, full=True)
    if not torch.cuda.is_available():                                                      # a valid call without a device: a status
        assert _call(lib) == _lib.ERR_HIP


# ------------------------------------------------------------------------------------------ GPU part
def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _truth(hidden, W, bias, w, mask):
    """torch float64 on the device -> (contributions [B, T, V], reps [B, V], logits [B, T, V]) of fp16 / fp32 operand VALUES."""
    import torch
    x = hidden.double() @ W.double().T
    if bias is not None:
        x = x + bias.double()
    p = torch.softmax(x, dim=-1)
    c = (p * w.double()[..., None]) * mask.double()[..., None]
    return c, c.max(dim=1).values, x


def _exact_on_device(B, L, V, H, seed):
    """the exact-arithmetic recipe (seeded on the CPU, so the truth is the same everywhere) -> hidden [B, L, H], W, bias fp32 on the device"""
    import torch
    rng = np.random.default_rng(seed)
    hidden = _dev((rng.integers(-8, 9, (B, L, H)) / 4).astype(np.float16))
    W = _dev((rng.choice(np.array([-1.0, 0.0, 0.0, 1.0]), (V, H)) / 8).astype(np.float16))
    bias = _dev((rng.integers(-16, 17, V) / 32).astype(np.float32))
    return hidden, W, bias, torch.Generator(device="cuda").manual_seed(seed)


def _assert_exact(x, hidden, W, bias):
    """the recipe's promise, on the truth: fp32 accumulation gives the float64 logits bit for bit, and they are fp16 values below 2^9."""
    x32 = hidden.float() @ W.float().T
    if bias is not None:
        x32 = x32 + bias.float()
    assert bool((x32.double() == x).all()) and bool((x.half().double() == x).all()) and float(x.abs().max()) < 2 ** 9


def _near_tie_slices(reps, tol, dims, remove):
    """slices whose two best groups lie within the sum of their tolerances -> bool [B, dims]"""
    B = reps.shape[0]
    g = reps[:, remove:].reshape(B, -1, dims)
    t = tol[:, remove:].reshape(B, -1, dims)
    order = np.argsort(-g, axis=1, kind="stable")[:, :2]
    top, tt = np.take_along_axis(g, order, 1), np.take_along_axis(t, order, 1)
    return (top[:, 0] - top[:, 1]) <= (tt[:, 0] + tt[:, 1])


def _vs_truth_and_parent(got16, parent16, truth, what):
    """fp16 record values against the truth (the midpoint rule) and bit for bit against the parent path's: both sides are roundings of
    values within the tolerance of the truth, so they may differ only where the truth is that close to an fp16 midpoint -> exemptions"""
    e_got = fp16_exemptions(got16, truth, what + " vs truth")
    e_parent = fp16_exemptions(parent16, truth, what + ": the parent path vs truth")
    differ = int((np.asarray(got16).view(np.uint16) != np.asarray(parent16).view(np.uint16)).sum())
    assert differ <= e_got + e_parent, what
    return e_got + differ


@pytest.mark.gpu
def test_goldens_on_gpu():
    import torch
    from dhr_amd import lexical_proj as LP
    g = _golden()
    for name in CASES:
        x = _exact_logits(g[name + "_hidden"], g[name + "_W"], g[name + "_bias"])
        w, mk = g[name + "_w"], g[name + "_mask"]
        ref, zero = g[name + "_reps"], reps_f64(x[:, 1:], w, mk[:, 1:])[1]
        cls = g[name + "_cls"]
        B, V = ref.shape
        dh = _dev(g[name + "_hidden"])[:, 1:]                                  # the strided view of the model's [B, L, H] states
        dW, db = _dev(g[name + "_W"]), _dev(g[name + "_bias"])
        dw, dm, dc = _dev(w), _dev(mk)[:, 1:], _dev(cls)
        for bias in (db, db.half()):
            rep = LP.lexical_reps(dh, dW, bias, dw, dm).cpu().numpy()
            check_f32(rep, ref, f"{name} reps")
            check_zero_signs(rep, ref, zero, f"{name} reps")
        dims, remove, agg = (int(v) for v in g[name + "_geom"])
        nc = cls.shape[1]
        if dims:
            rv = torch.full((B, dims + nc + 5), 7.0, dtype=torch.float16, device="cuda")
            ri = torch.full((B, dims + 3), 99, dtype=torch.uint8, device="cuda")
            LP.densify_lexical_into(dh, dW, db, dw, dm, rv[:, :dims + nc], ri[:, :dims], dims, remove, semantic_reps=dc)
            ref32 = np.concatenate([g[name + "_dval"], cls], 1)
            assert fp16_exemptions(rv[:, :dims + nc].cpu().numpy(), ref32, name) == 0
            assert np.array_equal(rv[:, :dims + nc].cpu().numpy().view(np.uint16), g[name + "_drec_v"].view(np.uint16))
            assert index_exemptions(ri[:, :dims].cpu().numpy(), ref, dims, remove, name) == 0
            assert np.array_equal(ri[:, :dims].cpu().numpy(), g[name + "_drec_i"])
            assert (rv[:, dims + nc:] == 7).all() and (ri[:, dims:] == 99).all()   # nothing beyond the record columns
        for full, key in ((True, "_afull"), (False, "_asemi")):
            av = torch.full((B, agg + nc + 2), 7.0, dtype=torch.float16, device="cuda")
            LP.aggregate_lexical_into(dh, dW, db, dw, dm, av[:, :agg + nc], agg, full=full, semantic_reps=dc)
            got = av.cpu().numpy()
            assert fp16_exemptions(got[:, :agg], g[name + key], name + key) == 0
            assert np.array_equal(got[:, :agg + nc].view(np.uint16), g[name + key + "_rec"].view(np.uint16)), (name, key)
            assert (got[:, agg + nc:] == 7).all()
            a32 = torch.zeros((B, agg), dtype=torch.float32, device="cuda")
            LP.aggregate_lexical_into(dh, dW, db, dw, dm, a32, agg, full=full)
            check_f32(a32.cpu().numpy(), g[name + key], name + key + " fp32")


@pytest.mark.gpu
def test_exact_operands_at_production_geometry():
    import torch
    from dhr_amd import lexical_proj as LP
    B, L, V, H, dims, remove, agg, nc = 5, 71, 30522, 768, 768, 570, 640, 24
    T = L - 1
    full_h, W, bias, gen = _exact_on_device(B, L, V, H, 31)
    hidden = full_h[:, 1:]
    w = torch.randn((B, T), generator=gen, device="cuda").half()
    lens = [T, 37, 0, 50, 23]                              # 70 | 107 | 107 | 157 | 180 rows: passages straddle the 64-row tiles
    mask = (torch.arange(T, device="cuda")[None] < torch.tensor(lens, device="cuda")[:, None]).long()
    mask[3, 10] = 0                                        # a masked token between unmasked ones
    cls = torch.randn((B, nc), generator=gen, device="cuda").half()
    entries = exempt = 0
    for bias_in in (bias, bias.half(), None):
        if bias_in is None or bias_in.dtype == torch.float32:
            c, truth, x = _truth(hidden, W, bias_in, w, mask)
            _assert_exact(x, hidden, W, bias_in)
            tn = truth.cpu().numpy()
            # no near-tie slice in the truth: where the two best groups lie within the tolerance they are EQUAL (the same token with the same
            # exact logit in two columns; the first group wins on both sides), so the group indices below must agree without exemptions
            top2 = -np.sort(-tn[:, remove:].reshape(B, -1, dims), axis=1)[:, :2]
            close = np.abs(top2[:, 0] - top2[:, 1]) <= 1e-5 * np.abs(top2[:, 0]) + 1e-30
            assert (top2[:, 0] == top2[:, 1])[close].all()
            zero = (c == 0).all(1).cpu().numpy()
            first = c[:, 0].float().cpu().numpy()          # where every contribution is zero, the first token's zero
            lg16 = x.half()                                # exact by construction: the parent path's input
            assert lens[2] == 0 and zero[2].all() and not zero[0].any()
            del c, x
        rep = LP.lexical_reps(hidden, W, bias_in, w, mask)
        check_f32(rep.cpu().numpy(), tn, "reps vs truth")
        check_zero_signs(rep.cpu().numpy(), first, zero, "reps")
        parent = LX.lexical_reps(lg16, w, mask)
        check_f32(parent.cpu().numpy(), tn, "parent reps vs truth")
        rv = torch.full((B, dims + nc + 8), 7.0, dtype=torch.float16, device="cuda")
        ri = torch.full((B, dims + 8), 99, dtype=torch.uint8, device="cuda")
        LP.densify_lexical_into(hidden, W, bias_in, w, mask, rv[:, :dims + nc], ri[:, :dims], dims, remove, semantic_reps=cls)
        pv = torch.zeros((B, dims + nc), dtype=torch.float16, device="cuda")
        pi = torch.zeros((B, dims), dtype=torch.uint8, device="cuda")
        LX.densify_lexical_into(lg16, w, mask, pv, pi, dims, remove, semantic_reps=cls)
        v64, i64 = densify_f64(tn, dims, remove)
        got = rv.cpu().numpy()
        exempt += _vs_truth_and_parent(got[:, :dims], pv[:, :dims].cpu().numpy(), v64, "densify values")
        entries += 2 * B * dims
        assert np.array_equal(got[:, dims:dims + nc], cls.cpu().numpy()) and (got[:, dims + nc:] == 7).all()
        assert np.array_equal(ri[:, :dims].cpu().numpy(), i64) and np.array_equal(pi.cpu().numpy(), i64) and (ri[:, dims:] == 99).all()
        r32 = torch.zeros((B, dims), dtype=torch.float32, device="cuda")
        i16 = torch.zeros((B, dims), dtype=torch.int16, device="cuda")
        LP.densify_lexical_into(hidden, W, bias_in, w, mask, r32, i16, dims, remove)
        check_f32(r32.cpu().numpy(), v64, "densify fp32")
        assert np.array_equal(i16.cpu().numpy(), i64)
        for full in (True, False):
            want = aggregate_f64(tn, agg, full)
            av = torch.full((B, agg + nc + 8), 7.0, dtype=torch.float16, device="cuda")
            LP.aggregate_lexical_into(hidden, W, bias_in, w, mask, av[:, :agg + nc], agg, full=full, semantic_reps=cls)
            pa = torch.zeros((B, agg), dtype=torch.float16, device="cuda")
            LX.aggregate_lexical_into(lg16, w, mask, pa, agg, full=full)
            got = av.cpu().numpy()
            exempt += _vs_truth_and_parent(got[:, :agg], pa.cpu().numpy(), want, "aggregate")
            entries += 2 * B * agg
            assert np.array_equal(got[:, agg:agg + nc], cls.cpu().numpy()) and (got[:, agg + nc:] == 7).all()
            a32 = torch.zeros((B, agg), dtype=torch.float32, device="cuda")
            LP.aggregate_lexical_into(hidden, W, bias_in, w, mask, a32, agg, full=full)
            check_f32(a32.cpu().numpy(), want, "aggregate fp32")
    print(f"exact operands: {exempt} midpoint exemptions in {entries} fp16 entries")
    assert exempt <= 5e-4 * entries


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,V,H,dims,remove,w_std", [(3, 24, 30522, 768, 768, 570, 0.02), (5, 19, 762, 72, 64, 58, 0.1)])
def test_inexact_operands_within_the_accumulation_bound(B, T, V, H, dims, remove, w_std):
    import torch
    from dhr_amd import lexical_proj as LP
    gen = torch.Generator(device="cuda").manual_seed(5 + H)
    hidden = torch.randn((B, T + 1, H), generator=gen, device="cuda").half()[:, 1:]
    W = (torch.randn((V, H), generator=gen, device="cuda") * w_std).half()
    bias = torch.randn((V,), generator=gen, device="cuda") * 0.1
    w = torch.randn((B, T), generator=gen, device="cuda").half()
    w[:, 0] = w[:, 0].abs() + 0.01                       # one positive weight per passage: no column's maximum is a padding zero (an exact tie)
    lens = torch.tensor([T, T // 2, 2, T - 3, 5][:B], device="cuda")
    mask = (torch.arange(T, device="cuda")[None] < lens[:, None]).long()
    c, truth, _ = _truth(hidden, W, bias, w, mask)
    A = ((hidden.double().abs() @ W.double().abs().T) + bias.double().abs()).max(dim=-1).values                  # [B, T]
    tol = (c.abs() * (2 * (H + 2) * 2.0 ** -24 * A + 1e-5)[..., None]).max(dim=1).values.cpu().numpy()           # [B, V]
    tn = truth.cpu().numpy()
    rep = LP.lexical_reps(hidden, W, bias, w, mask).cpu().numpy().astype(np.float64)
    err = np.abs(rep - tn)
    print(f"H={H} V={V}: reps error / bound: max {np.max(err / np.maximum(tol, 1e-300)):.3f}")
    assert (err <= tol).all(), f"{(err > tol).sum()} reps outside the bound, worst {np.max(err / np.maximum(tol, 1e-300)):.2f}x"
    # densified records: the truth first (few slices whose best two groups the bound cannot tell apart), then the kernel
    near = _near_tie_slices(tn, tol, dims, remove)
    print(f"H={H} V={V}: {near.mean():.4f} of the slices are near-ties of the truth")
    assert near.mean() <= 0.02
    v64, i64 = densify_f64(tn, dims, remove)
    tol_d = tol[:, remove:].reshape(B, -1, dims).max(1)
    rv = torch.zeros((B, dims), dtype=torch.float16, device="cuda")
    ri = torch.zeros((B, dims), dtype=torch.uint8, device="cuda")
    LP.densify_lexical_into(hidden, W, bias, w, mask, rv, ri, dims, remove)
    got = rv.cpu().numpy()
    half_ulp = 0.5 * np.spacing(np.abs(v64).astype(np.float16)).astype(np.float64)
    assert (np.abs(got.astype(np.float64) - v64) <= tol_d + half_ulp).all()
    assert (ri.cpu().numpy() == i64)[~near].all()
    r32 = torch.zeros((B, dims), dtype=torch.float32, device="cuda")
    LP.densify_lexical_into(hidden, W, bias, w, mask, r32, ri, dims, remove)
    assert (np.abs(r32.cpu().numpy().astype(np.float64) - v64) <= tol_d).all()


@pytest.mark.gpu
def test_zeros_keep_their_signs():
    """Negative term weights with padding and a fully masked passage: a masked token folds in (p * w) * 0, and the first zero in token
    order decides the sign of a zero maximum."""
    import torch
    from dhr_amd import lexical_proj as LP
    B, L, V, H = 7, 10, 202, 24
    T = L - 1
    full_h, W, bias, gen = _exact_on_device(B, L, V, H, 77)
    hidden = full_h[:, 1:]
    w = -torch.rand((B, T), generator=gen, device="cuda").half() - 0.25
    mask = torch.ones((B, T), dtype=torch.long, device="cuda")
    mask[1, 4:] = 0                                        # padding behind negative contributions: -0 wins
    mask[2, :] = 0                                         # fully masked: the first token's zero
    mask[3, :] = 0
    w[3, 0] = 0.5                                          # ... +0 when its weight is positive
    mask[4, 2] = 0                                         # a masked token between unmasked ones,
    w[4, 2] = 0.75                                         # with a positive weight: +0
    mask[5, 0] = 0                                         # the first token masked, -0; a later masked token with w > 0 does not replace it
    mask[5, 6] = 0
    w[5, 6] = 1.0
    w[6] = w[6].abs()                                      # positive contributions, padding: the zeros never win
    mask[6, 5:] = 0
    x = _exact_logits(hidden.cpu().numpy(), W.cpu().numpy(), bias.cpu().numpy())
    c = contributions_f64(x, w.float().cpu().numpy(), mask.cpu().numpy())
    ref = _first_max(c)
    zero = ref == 0
    assert zero[1:6].all() and not zero[0].any() and not zero[6].any()
    assert np.signbit(ref[1]).all() and np.signbit(ref[2]).all() and not np.signbit(ref[3]).any() and not np.signbit(ref[4]).any() and np.signbit(ref[5]).all()
    rep = LP.lexical_reps(hidden, W, bias, w, mask).cpu().numpy()
    check_f32(rep, ref, "reps")
    check_zero_signs(rep, ref, zero, "reps")
    want = aggregate_f64(ref, 8, True).astype(np.float32)
    a32 = torch.zeros((B, 8), dtype=torch.float32, device="cuda")
    LP.aggregate_lexical_into(hidden, W, bias, w, mask, a32, 8, full=True)
    assert np.array_equal(a32.cpu().numpy().view(np.uint32)[want == 0], want.view(np.uint32)[want == 0])
    check_f32(a32.cpu().numpy(), want, "aggregate")
    with pytest.raises(_lib.DhrError, match="dtype"):
        LP.lexical_reps(hidden.float(), W.float(), bias, w, mask)
    with pytest.raises(_lib.DhrError, match="dtype"):
        LP.lexical_reps(hidden, W, bias.double(), w, mask)
    with pytest.raises(_lib.DhrError, match="multiple of 8"):
        LP.lexical_reps(hidden[..., :20], W[:, :20], bias, w, mask)


@pytest.mark.gpu
def test_two_calls_are_bit_identical_and_memory_stays_within_the_workspace_bound():
    import torch
    from dhr_amd import lexical_proj as LP
    B, T, V, H, dims, remove = 16, 64, 30522, 768, 768, 570
    gen = torch.Generator(device="cuda").manual_seed(3)
    hidden = torch.randn((B, T, H), generator=gen, device="cuda").half()
    W = (torch.randn((V, H), generator=gen, device="cuda") * 0.02).half()
    bias = (torch.randn((V,), generator=gen, device="cuda") * 0.1).half()
    w = torch.randn((B, T), generator=gen, device="cuda")
    mask = (torch.arange(T, device="cuda")[None] < torch.randint(1, T + 1, (B, 1), generator=gen, device="cuda")).float()
    outs = [(torch.zeros((B, dims), dtype=torch.float16, device="cuda"), torch.zeros((B, dims), dtype=torch.uint8, device="cuda")) for _ in range(2)]
    reps = [torch.zeros((B, V), dtype=torch.float32, device="cuda") for _ in range(2)]
    LP.densify_lexical_into(hidden, W, bias, w, mask, outs[0][0], outs[0][1], dims, remove)       # (loads the library, warms the allocator)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    LP.densify_lexical_into(hidden, W, bias, w, mask, outs[1][0], outs[1][1], dims, remove)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"B={B} T={T}: peak rise {rise / 1e6:.2f} MB, bound {_bound(B, T, V) / 1e6:.2f} MB, the logits would be {B * T * V * 2 / 1e6:.1f} MB")
    assert rise <= _bound(B, T, V)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    for r in reps:
        r.copy_(LP.lexical_reps(hidden, W, bias, w, mask))
    assert torch.equal(reps[0].view(torch.int32), reps[1].view(torch.int32))


@pytest.mark.gpu
def test_timing_printout():
    """The fused op (densify mode into fp16 records) vs the parent composition on the same inputs, torch.nn.functional.linear in fp16
    followed by lexical.densify_lexical_into: device events, 3 warm-ups, median of 10.  A printout, not a threshold."""
    import torch
    from dhr_amd import lexical_proj as LP
    V, H, dims, remove = 30522, 768, 768, 570
    W = (torch.randn((V, H), device="cuda") * 0.02).half()
    bias = (torch.randn((V,), device="cuda") * 0.1).half()
    for B, L in ((128, 128), (128, 32)):
        hidden = torch.randn((B, L, H), device="cuda").half()[:, 1:]
        w = torch.randn((B, L - 1), device="cuda").half()
        mask = torch.ones((B, L - 1), dtype=torch.long, device="cuda")
        rv = torch.empty((B, dims), dtype=torch.float16, device="cuda")
        ri = torch.empty((B, dims), dtype=torch.uint8, device="cuda")

        def fused():
            LP.densify_lexical_into(hidden, W, bias, w, mask, rv, ri, dims, remove)

        def parent():
            LX.densify_lexical_into(torch.nn.functional.linear(hidden, W, bias), w, mask, rv, ri, dims, remove)

        res = {}
        for name, fn in (("fused", fused), ("parent", parent)):
            for _ in range(3):
                fn()
            times = []
            for _ in range(10):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            res[name] = float(np.median(times))
        print(f"lexical projection head B={B} L={L} fp16, all tokens unmasked: fused {res['fused']:.3f} ms, linear + head {res['parent']:.3f} ms, "
              f"{res['parent'] / res['fused']:.2f}x")
        del hidden
        torch.cuda.empty_cache()
