"""The differentiable lexical head (dhr_amd/lexical_train.py on dhr_lexical_head_train / dhr_lexical_head_backward, dhr_amd/csrc/lexical_train.hip)
against the reference's own encoder code under autograd (tests/golden/lexical_train_golden.npz, made by tests/golden/make_golden_lexical_train.py),
a float64 restatement kept here that shares no code with the library, and the eager torch composition on the same device.

Routing.  A (b, v) entry is a near-tie when some token's float64 contribution lies within 1e-5 * |max| + 1e-30 of the maximum without being
equal to it (the tolerance of tests/test_lexical_head.py).  Everywhere else the library's tok must equal the float64 first-argmax (on an
exact tie the first token).  At a near-tie it may name any token within that tolerance, and the gradient truth is built with the token it
named.  Near-ties are counted: zero on the goldens, at most 1e-4 of the (b, v) entries on random data.

Gradient values: no absolute term, no hand-picked rtol.  With u = 2^-24, p the float64 softmax, d = max_v x - x, dbar = sum_v p d, every fp32
evaluation of p = exp(x - max) / sum carries a relative error of at most kappa * u,

    kappa[b,t,v] = 8 + d + dbar + 2 s,     s = ceil(V / 1024) + 10

 - x - max rounds once, which moves exp by a relative d * u; expf is good to 1 ulp = 2 u: (2 + d) u for the numerator;
 - the normaliser is a sum of such terms, (2 + dbar) u, plus its own roundings: one if it is accumulated in fp64 (this library), up to s for an
   fp32 sum by a 1024-thread block (a sequential chunk of ceil(V / 1024) terms per thread, then a 10-level tree: the eager composition);
 - the division, or the reciprocal and the product, and one spare: 3 u; the second s covers an fp32 softmax kept by autograd and read again.
With R = [tok == t] g w m the routed term, S1[b,t] = sum over the routed v' of |g p w m| and kr[b,t] the largest kappa among them:
 - D = w m A: the errors of the p inside A (kr u S1), the rounding of A or of an fp32 sum over the vocabulary (s u S1), w * m and the product
   (2 u S1); R: 2 u |R|; the subtraction: u (|R| + S1); the product with p and its rounding: (kappa + 1) u (|R| + S1).  Together
       |dL/dx - truth| <= k u p (|R| + S1),        k[b,t,v] = kappa + kr + s + 5
 - dL/dw = m A:  |dL/dw - truth| <= k u |m| sum |g p|,   k[b,t] = kr + s + 3
plus the fp16 rounding of the truth where the output is fp16: 2^-11 |truth|, and 2^-25 below the normal range (half the spacing of the fp16
subnormals: gradients under 6e-8 flush, in the eager composition as well, which is why fp16 training scales its loss).  Where the truth and
the bound are zero (skipped and masked tokens, -inf logits) the result must be exactly zero.  The eager torch composition is held to the same bound in the same tests.  Measured worst error / bound on an MI355X where the
output is fp32: 0.08 (dL/dlogits) and 0.01 (dL/dw) for this library, 0.13 and 0.01 for the eager composition; where it is fp16 the rounding of
the output decides and both sit just below 1 (profiles/lexical_train.txt).

CPU part (-m "not gpu"): the fixture against the restatement; statuses of the three entry points; the wrapper's errors.  GPU part: goldens,
seeded random cases (views and skip_tokens bit-identical), two backward runs bit-identical, a composed training step, memory, timing."""
import os

import numpy as np
import pytest

from dhr_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "lexical_train_golden.npz")
CASES = ("prod", "small", "neg")
U32, U16, SUB16 = 2.0 ** -24, 2.0 ** -11, 2.0 ** -25
RTOL, ATOL = 1e-5, 1e-30
NEW_SYMBOLS = ("dhr_lexical_head_train_workspace", "dhr_lexical_head_train", "dhr_lexical_head_backward")


# ------------------------------------------------------------------------------------------ float64 restatement
def softmax64(logits):
    """-> (p, d) float64 [B, T, V]: the softmax over the vocabulary and max - x (0 where p is 0)"""
    x = np.asarray(logits).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = x.max(-1, keepdims=True) - x
        e = np.exp(-d)
        p = e / e.sum(-1, keepdims=True)
    p = np.where(np.isnan(p), 0.0, p)
    return p, np.where(p > 0, d, 0.0)


def forward64(logits, w, m):
    """-> (p, d, reps [B, V], first maximising token [B, V], near-tie flags [B, V], contributions [B, T, V])"""
    p, d = softmax64(logits)
    c = (p * np.asarray(w, np.float64)[..., None]) * np.asarray(m, np.float64)[..., None]
    r, a = c[:, 0].copy(), np.zeros(c[:, 0].shape, np.int64)
    for t in range(1, c.shape[1]):
        up = c[:, t] > r
        r, a = np.where(up, c[:, t], r), np.where(up, t, a)
    near = (((r[:, None] - c) <= RTOL * np.abs(r[:, None]) + ATOL) & (c != r[:, None])).any(1)
    return p, d, r, a, near, c


def backward64(p, d, w, m, G, tok):
    """The formulas of the issue with the routing `tok`.  -> (dx, bound_dx [B, T, V], dw, bound_dw [B, T])"""
    w, m, G = np.asarray(w, np.float64), np.asarray(m, np.float64), np.asarray(G, np.float64)
    B, T, V = p.shape
    s = -(-V // 1024) + 10
    route = np.asarray(tok, np.int64)[:, None, :] == np.arange(T)[None, :, None]
    gp = route * G[:, None, :] * p
    A = gp.sum(-1)
    dw, D = m * A, w * m * A
    R = route * G[:, None, :] * (w * m)[..., None]
    dx = p * (R - D[..., None])
    kappa = 8 + d + (p * d).sum(-1, keepdims=True) + 2 * s
    kr = np.where(gp != 0, kappa, 0.0).max(-1)
    S1g = np.abs(gp).sum(-1)
    S1 = np.abs(w * m) * S1g
    b_dx = (kappa + kr[..., None] + s + 5) * U32 * p * (np.abs(R) + S1[..., None])
    b_dw = (kr + s + 3) * U32 * np.abs(m) * S1g
    return dx, b_dx, dw, b_dw


def assert_within(got, truth, bound, what, fp16=False):
    got = np.asarray(got).astype(np.float64)
    assert got.shape == truth.shape, (what, got.shape, truth.shape)
    tol = bound + (np.where(truth != 0, np.maximum(U16 * np.abs(truth), SUB16), 0.0) if fp16 else 0.0)
    err = np.abs(got - truth)
    bad = ~(err <= tol)
    worst = float((err / np.where(tol > 0, tol, 1.0))[tol > 0].max()) if (tol > 0).any() else 0.0
    worst32 = float((err / np.where(bound > 0, bound, 1.0))[bound > 0].max()) if (bound > 0).any() else 0.0
    print(f"{what}: max error / bound = {worst:.4f} (against the fp32 part alone {worst32:.4f}), entries with a zero bound that are not zero: "
          f"{int((err[tol == 0] != 0).sum())}")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} entries outside the bound (worst error / bound {worst:.3f})"
    return worst


def check_routing(tok, a, near, c, what):
    """tok equals the float64 first-argmax outside near-ties; at a near-tie it names a token within the tolerance.  -> near-tie count"""
    tok = np.asarray(tok, np.int64)
    assert tok.min() >= 0 and tok.max() < c.shape[1], what
    diff = tok != a
    assert not (diff & ~near).any(), f"{what}: {int((diff & ~near).sum())} tokens differ from the float64 first-argmax outside near-ties"
    top = c.max(1)
    named = np.take_along_axis(c, tok[:, None, :], 1)[:, 0]
    assert ((top - named) <= RTOL * np.abs(top) + ATOL).all(), f"{what}: a named token is not within the tolerance of the maximum"
    return int(near.sum())


def _golden():
    return np.load(GOLDEN)


def _case(g, name):
    """-> full logits [B, L, V] fp16, w [B, L-1], mask [B, L-1] (of the tokens after [CLS]), reps, G, dlogits [B, L, V], dw"""
    return (g[name + "_logits"], g[name + "_w"], g[name + "_mask"][:, 1:], g[name + "_reps"], g[name + "_G"], g[name + "_dlogits"], g[name + "_dw"])


# ------------------------------------------------------------------------------------------ CPU part
def test_fixture_matches_float64_restatement():
    g = _golden()
    for name in CASES:
        lg, w, m, reps, G, dlg, dw = _case(g, name)
        p, d, r, a, near, _ = forward64(lg[:, 1:], w, m)
        assert not near.any(), name                                               # the goldens hold no near-tie: no exemption below
        assert np.all(np.abs(reps - r) <= RTOL * np.abs(r) + ATOL), name
        dx64, b_dx, dw64, b_dw = backward64(p, d, w, m, G, a)
        assert_within(dlg[:, 1:], dx64, b_dx, name + " dL/dlogits (fixture)")
        assert_within(dw, dw64, b_dw, name + " dL/dw (fixture)")
        assert not dlg[:, 0].any(), name                                          # token 0 is dropped: its gradient is exactly zero
        assert not dlg[:, 1:][m == 0].any() and not dw[m == 0].any(), name        # masked tokens: exactly zero
        assert (G == 0).any() and (G < 0).any() and (G > 0).any()
    # the cases cover what they were designed for
    sm = g["small_logits"]
    assert g["prod_logits"].shape[2] == 30522 and np.array_equal(sm[1, 2], sm[1, 4]) and g["small_w"][1, 1] == g["small_w"][1, 3]
    assert np.isneginf(sm).any() and (g["small_mask"][3, 1:] == 0).all() and (g["small_mask"][0, 5:] == 0).all() and (g["neg_w"] < 0).all()
    _, _, _, a, _, _ = forward64(sm[:, 1:], g["small_w"], g["small_mask"][:, 1:])
    assert (a[1] != 3).all() and (a[1] == 1).any()                                # the exact token tie: the first of the two takes the route
    assert g["small_dlogits"][1, 2].any() and not g["small_dlogits"][1, 4][a[1] == 1].any()
    assert os.path.getsize(GOLDEN) < 512 * 1024


def _train_args(**kw):
    a = dict(device=0, mem_kind=_lib.MEM_DEVICE, logits=_A["lg"].ctypes.data, dtype=_lib.VAL_F16, batch=2, n_tokens=3, skip=1, vocab=32, ld_batch=128,
             ld_token=32, w=_A["w"].ctypes.data, ld_w=3, m=_A["m"].ctypes.data, ld_m=3, reps=_A["reps"].ctypes.data, ld_reps=32, tok=_A["tok"].ctypes.data,
             ld_tok=32, ws=_A["ws"].ctypes.data, stream=None)
    a.update(kw)
    return list(a.values())


def _bwd_args(**kw):
    a = dict(device=0, mem_kind=_lib.MEM_DEVICE, logits=_A["lg"].ctypes.data, dtype=_lib.VAL_F16, batch=2, n_tokens=3, skip=1, vocab=32, ld_batch=128,
             ld_token=32, g=_A["g"].ctypes.data, ld_g=32, tok=_A["tok"].ctypes.data, ld_tok=32, ws=_A["ws"].ctypes.data, dx=_A["dx"].ctypes.data,
             ld_dx_batch=128, ld_dx_token=32, dw=_A["dw"].ctypes.data, ld_dw=3, stream=None)
    a.update(kw)
    return list(a.values())


_A = dict(lg=np.zeros((2, 4, 32), np.float16), w=np.ones((2, 3), np.float32), m=np.ones((2, 3), np.float32), reps=np.zeros((2, 32), np.float32),
          tok=np.zeros((2, 32), np.int16), ws=np.zeros(2 * 3 * 20, np.uint8), g=np.ones((2, 32), np.float32), dx=np.zeros((2, 4, 32), np.float16),
          dw=np.zeros((2, 3), np.float32))


def test_entry_points_return_statuses():
    import torch
    lib = _lib.load()
    assert lib.dhr_lexical_head_train_workspace(2, 3) == 2 * 3 * 20
    assert lib.dhr_lexical_head_train_workspace(192, 149) == 192 * 149 * 20
    for b, t in ((0, 3), (-1, 3), (2, 0), (2, -5), (2, 32768)):
        assert lib.dhr_lexical_head_train_workspace(b, t) == 0
    bad = [dict(logits=None), dict(w=None), dict(m=None), dict(reps=None), dict(tok=None), dict(ws=None), dict(mem_kind=7), dict(dtype=5),
           dict(n_tokens=0), dict(n_tokens=-2), dict(skip=-1), dict(skip=40000), dict(vocab=0), dict(ld_token=31), dict(ld_batch=127), dict(skip=2),
           dict(ld_w=2), dict(ld_m=2), dict(ld_reps=31), dict(ld_tok=31), dict(batch=-1)]
    for b in bad:
        assert lib.dhr_lexical_head_train(*_train_args(**b)) == _lib.ERR_INVALID, b
    bad = [dict(logits=None), dict(g=None), dict(tok=None), dict(ws=None), dict(mem_kind=7), dict(dtype=5), dict(n_tokens=0), dict(skip=-1),
           dict(skip=2), dict(vocab=0), dict(ld_token=31), dict(ld_batch=127), dict(ld_g=31), dict(ld_tok=31), dict(ld_dx_token=31),
           dict(ld_dx_batch=127), dict(ld_dw=2), dict(batch=-1)]
    for b in bad:
        assert lib.dhr_lexical_head_backward(*_bwd_args(**b)) == _lib.ERR_INVALID, b
    # more tokens than the int16 token index holds, and host arrays: statuses with a message, no staging path
    assert lib.dhr_lexical_head_train(*_train_args(n_tokens=32768, ld_batch=1 << 21, ld_w=32768, ld_m=32768)) == _lib.ERR_UNSUPPORTED
    assert lib.dhr_lexical_head_train(*_train_args(mem_kind=_lib.MEM_HOST)) == _lib.ERR_UNSUPPORTED
    assert lib.dhr_lexical_head_backward(*_bwd_args(mem_kind=_lib.MEM_HOST)) == _lib.ERR_UNSUPPORTED
    assert b"live on the device" in lib.dhr_last_error()
    # nothing to do: no device is touched
    assert lib.dhr_lexical_head_train(*_train_args(batch=0)) == _lib.DHR_OK
    assert lib.dhr_lexical_head_backward(*_bwd_args(batch=0)) == _lib.DHR_OK
    assert lib.dhr_lexical_head_backward(*_bwd_args(dx=None, dw=None)) == _lib.DHR_OK
    # valid calls: a status without a device, the result with one
    if not torch.cuda.is_available():
        assert lib.dhr_lexical_head_train(*_train_args()) == _lib.ERR_HIP
        assert lib.dhr_lexical_head_backward(*_bwd_args()) == _lib.ERR_HIP
        return
    t = {k: torch.from_numpy(v).cuda() for k, v in _A.items()}
    ptr = {k: v.data_ptr() for k, v in t.items()}
    assert lib.dhr_lexical_head_train(*_train_args(logits=ptr["lg"], w=ptr["w"], m=ptr["m"], reps=ptr["reps"], tok=ptr["tok"], ws=ptr["ws"])) == _lib.DHR_OK
    assert lib.dhr_lexical_head_backward(*_bwd_args(logits=ptr["lg"], g=ptr["g"], tok=ptr["tok"], ws=ptr["ws"], dx=ptr["dx"], dw=ptr["dw"])) == _lib.DHR_OK
    torch.cuda.synchronize()
    assert torch.equal(t["reps"], torch.full((2, 32), 1 / 32, device="cuda")) and not t["tok"].any() and not t["dx"][:, 0].any()


def test_wrapper_raises_before_touching_the_library(monkeypatch):
    import torch
    from dhr_amd import lexical_train as LT

    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", no_library)
    lg, w, m = torch.zeros((2, 5, 32), dtype=torch.float16), torch.ones((2, 4)), torch.ones((2, 4), dtype=torch.long)
    for args in ((lg[0], w, m, 1), (lg[None], w, m, 1), (lg, w, m, 0), (lg, w[:, :3], m, 1), (lg, w, m[:, :3], 1), (lg, w[..., None, None], m, 1),
                 (lg, w, m, 5), (lg, w, m, 7), (lg, w, m, -1), (lg[:, :0], w[:, :0], m[:, :0], 0)):
        with pytest.raises(ValueError):
            LT.lexical_reps(*args)
    with pytest.raises(ValueError, match="no tokens"):
        LT.lexical_reps(lg, w, m, skip_tokens=5)
    for args in ((lg.double(), w, m, 1), (lg.to(torch.bfloat16), w, m, 1), (lg, w.long(), m, 1), (lg.numpy(), w.numpy(), m.numpy(), 1)):
        with pytest.raises(_lib.DhrError):
            LT.lexical_reps(*args)
    with pytest.raises(_lib.DhrError, match="GPU"):                               # CPU tensors: there is no CPU implementation
        LT.lexical_reps(lg, w, m, skip_tokens=1)
    with pytest.raises(_lib.DhrError, match="GPU"):
        LT.lexical_reps(lg, w[..., None], m[..., None], skip_tokens=1, return_tokens=True)


def test_new_symbols_are_declared_everywhere():
    header = open(os.path.join(HERE, "..", "include", "dhr_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and name + "(" in header
        getattr(lib, name)
    # the version script exports the dhr_ prefix and nothing else
    vmap = open(os.path.join(HERE, "..", "dhr_amd", "csrc", "libdhr.map")).read()
    assert "dhr_*;" in vmap and "local:" in vmap


# ------------------------------------------------------------------------------------------ GPU part
def _eager(full, w, mask, skip=1):
    """The reference's lines on the device with autograd (fp32 softmax as under autocast).  -> (reps, tok)"""
    import torch
    p = torch.softmax(full[:, skip:].float(), dim=-1)
    r = torch.max((p * w.reshape(w.shape[0], -1, 1)) * mask.reshape(mask.shape[0], -1, 1), dim=-2)
    return r.values, r.indices


def _np(t):
    return t.detach().float().cpu().numpy()


def _check_grads(tag, p, d, w, m, G, tok, dx, dw, x_fp16, w_fp16):
    dx64, b_dx, dw64, b_dw = backward64(p, d, w, m, G, tok)
    rx = assert_within(dx, dx64, b_dx, tag + " dL/dlogits", fp16=x_fp16)
    rw = assert_within(dw, dw64, b_dw, tag + " dL/dw", fp16=w_fp16)
    return rx, rw


@pytest.mark.gpu
def test_goldens_on_gpu():
    import torch
    from dhr_amd import lexical as LX
    from dhr_amd import lexical_train as LT
    g = _golden()
    for name in CASES:
        lg, w, m, reps, G, dlg, dw = _case(g, name)
        p, d, r, a, near, c = forward64(lg[:, 1:], w, m)
        for dt in (torch.float16, torch.float32):
            full = torch.from_numpy(lg).to("cuda", dt).requires_grad_(True)
            tw = torch.from_numpy(w).cuda()[..., None].requires_grad_(True)       # [B, T, 1], as term_weight_trans returns it
            tm = torch.from_numpy(m).cuda()
            out, tok = LT.lexical_reps(full, tw, tm, skip_tokens=1, return_tokens=True)
            assert out.dtype == torch.float32 and tok.dtype == torch.int16 and out.requires_grad and not tok.requires_grad
            enc = LX.lexical_reps(full[:, 1:], tw, tm)
            assert torch.equal(out.detach().view(torch.int32), enc.view(torch.int32)), name          # bit-equal to the encoding head
            assert check_routing(tok.cpu().numpy(), a, near, c, name) == 0
            assert np.array_equal(tok.cpu().numpy(), a), name
            out.backward(torch.from_numpy(G).cuda())
            assert full.grad.dtype == dt and full.grad.shape == full.shape and tw.grad.shape == tw.shape
            gx = _np(full.grad)
            assert not gx[:, 0].any() and not gx[:, 1:][m == 0].any() and not _np(tw.grad)[..., 0][m == 0].any()
            _check_grads(f"{name} {dt}", p, d, w, m, G, a, gx[:, 1:], _np(tw.grad)[..., 0], dt == torch.float16, False)
            # ... and against what the reference's autograd returned, each within the bound of the truth
            _, b_dx, _, b_dw = backward64(p, d, w, m, G, a)
            assert np.all(np.abs(gx[:, 1:] - dlg[:, 1:]) <= 2 * b_dx + (np.maximum(U16 * np.abs(dlg[:, 1:]), SUB16) if dt == torch.float16 else 0))
            assert np.all(np.abs(_np(tw.grad)[..., 0] - dw) <= 2 * b_dw)


RANDOM = [  # B, L, V, logits dtype, weights dtype, strided base, positive weights
    (3, 9, 1082, "float16", "float16", False, False),
    (4, 17, 4027, "float32", "float32", True, False),
    (2, 150, 30522, "float16", "float16", False, True),
    (5, 2, 203, "float32", "float16", False, False),
    (3, 32, 30522, "float16", "float32", True, False),
    (3, 12, 203, "float16", "float16", True, True),
    # ceil(T / 16) * B = 512 workgroups: the backward's reduction pass takes 16 tokens per workgroup.  Rows of 8 columns take the multi-dword
    # accesses of the streaming pass, the 18-byte fp16 rows of 9 columns and rows below 8 columns (any dtype) the element-wise ones
    (512, 3, 8, "float16", "float32", False, False),
    (512, 3, 9, "float16", "float32", False, False),
    (512, 3, 8, "float32", "float32", False, False),
    (512, 3, 7, "float32", "float32", False, False),
]


def _random_case(gen, B, L, V, ldt, wdt, strided, positive):
    """-> (leaf holding the model's [B, L, V] logits (see _full), its dtype, w [B, L-1, 1], mask [B, L-1], G [B, V])"""
    import torch
    ldt, wdt = getattr(torch, ldt), getattr(torch, wdt)
    shape = (B + 1, L + 2, V + 6) if strided else (B, L, V)
    leaf = (torch.randn(shape, generator=gen, device="cuda") * 2).to(ldt).requires_grad_(True)
    w = torch.randn((B, L - 1, 1), generator=gen, device="cuda")
    w = (w.abs() if positive else w).to(wdt).requires_grad_(True)
    mask = torch.ones((B, L - 1), dtype=torch.int64, device="cuda")
    mask[0, (L - 1) // 2:] = 0
    if B > 2:
        mask[-1, :] = 0                                                           # a fully masked row
    G = torch.randn((B, V), generator=gen, device="cuda")
    G = G * (torch.rand((B, V), generator=gen, device="cuda") > 0.1)             # mixed signs, a tenth zeros
    return leaf, ldt, w, mask, G


def _full(leaf, B, L, V, strided):
    return leaf[1:, 1:L + 1, 2:V + 2] if strided else leaf


@pytest.mark.gpu
def test_random_cases_views_and_skip_tokens():
    import torch
    from dhr_amd import lexical as LX
    from dhr_amd import lexical_train as LT
    gen = torch.Generator(device="cuda").manual_seed(17)
    entries = ties = 0
    worst = {}                                                                    # (who, dtype of the output) -> worst error / bound

    def note(who, dtype, ratio):
        worst[who, dtype] = max(worst.get((who, dtype), 0.0), ratio)

    for k, (B, L, V, ldt, wdt, strided, positive) in enumerate(RANDOM):
        leaf, dt, w, mask, G = _random_case(gen, B, L, V, ldt, wdt, strided, positive)
        tag = f"random[{k}] {B}x{L}x{V} {ldt}"
        runs = []
        for skip in (1, 0):
            leaf.grad = w.grad = None
            full = _full(leaf, B, L, V, strided)
            out, tok = LT.lexical_reps(full if skip else full[:, 1:], w, mask, skip_tokens=skip, return_tokens=True)
            out.backward(G)
            runs.append((out.detach(), tok, leaf.grad, w.grad))
        for x, y in zip(*runs):                                                   # the view and skip_tokens=1: the same bits
            assert torch.equal(x, y), tag
        out, tok, gleaf, gw = runs[0]
        full = _full(leaf, B, L, V, strided).detach()
        assert torch.equal(out.view(torch.int32), LX.lexical_reps(full[:, 1:], w, mask).view(torch.int32)), tag
        gfull = _full(gleaf, B, L, V, strided)
        assert gleaf.dtype == dt and gw.dtype == w.dtype and gw.shape == w.shape
        assert not gfull[:, 0].any() and int((gleaf != 0).sum()) == int((gfull != 0).sum()), tag      # nothing outside the view, token 0 zero
        xn, wn, mn, Gn = _np(full)[:, 1:], _np(w)[..., 0], mask.cpu().numpy(), _np(G)
        p, d, r, a, near, c = forward64(xn, wn, mn)
        ties += check_routing(tok.cpu().numpy(), a, near, c, tag)
        entries += B * V
        assert np.all(np.abs(_np(out) - r) <= RTOL * np.abs(r) + ATOL), tag
        assert not _np(gfull)[:, 1:][mn == 0].any() and not _np(gw)[..., 0][mn == 0].any(), tag
        rx, rw = _check_grads(tag, p, d, wn, mn, Gn, tok.cpu().numpy(), _np(gfull)[:, 1:], _np(gw)[..., 0], ldt == "float16", wdt == "float16")
        note("library dL/dlogits", ldt, rx)
        note("library dL/dw", wdt, rw)
        # the eager torch composition with autograd on the same device: the same bound
        leaf.grad = w.grad = None
        e_out, e_tok = _eager(_full(leaf, B, L, V, strided), w, mask)
        e_out.backward(G)
        check_routing(e_tok.cpu().numpy(), a, near, c, tag + " eager")
        rx, rw = _check_grads(tag + " eager", p, d, wn, mn, Gn, e_tok.cpu().numpy(), _np(_full(leaf.grad, B, L, V, strided))[:, 1:], _np(w.grad)[..., 0],
                              ldt == "float16", wdt == "float16")
        note("eager dL/dlogits", ldt, rx)
        note("eager dL/dw", wdt, rw)
        del leaf, gleaf, runs
        torch.cuda.empty_cache()
    print(f"random: {ties} near-ties in {entries} (b, v) entries; worst error / bound: " + ", ".join(f"{a} {b} {r:.4f}" for (a, b), r in sorted(worst.items())))
    assert ties <= 1e-4 * entries


@pytest.mark.gpu
def test_two_backward_runs_are_bit_identical():
    import torch
    from dhr_amd import lexical_train as LT
    gen = torch.Generator(device="cuda").manual_seed(23)
    for B, L, V, ldt in ((4, 40, 30522, "float16"), (3, 150, 4027, "float32")):
        leaf, dt, w, mask, G = _random_case(gen, B, L, V, ldt, "float32", False, False)
        runs = []
        for _ in range(2):
            leaf.grad = w.grad = None
            LT.lexical_reps(leaf, w, mask, skip_tokens=1).backward(G)
            runs.append((leaf.grad.clone(), w.grad.clone()))
        out = LT.lexical_reps(leaf, w, mask, skip_tokens=1)                        # ... and twice through one graph
        out.backward(G, retain_graph=True)
        leaf.grad = w.grad = None
        out.backward(G)
        runs.append((leaf.grad, w.grad))
        for gx, gw in runs[1:]:
            assert torch.equal(gx.view(torch.int16 if dt == torch.float16 else torch.int32), runs[0][0].view(torch.int16 if dt == torch.float16 else torch.int32))
            assert torch.equal(gw.view(torch.int32), runs[0][1].view(torch.int32))
        # only one of the two gradients asked for
        x2, w2 = leaf.detach().clone().requires_grad_(True), w.detach().clone()
        LT.lexical_reps(x2, w2, mask, skip_tokens=1).backward(G)
        assert torch.equal(x2.grad, runs[0][0])
        x3, w3 = leaf.detach().clone(), w.detach().clone().requires_grad_(True)
        LT.lexical_reps(x3, w3, mask, skip_tokens=1).backward(G)
        assert torch.equal(w3.grad, runs[0][1])


@pytest.mark.gpu
def test_composed_training_step():
    """Stub logits -> lexical reps of queries and passages -> listwise_gip_scores -> the reference's KL loss against one-hot labels
    (tevatron/DHR/modeling.py:189-197) -> backward, with this head and with the eager head.  The upstream dL/dreps of the two steps differ by
    the roundings of their reps, so each step is held to the bound of the truth under ITS OWN dL/dreps and routing: two results that both lie
    inside that bound are as close as fp32 lets them be.  The losses agree to 1e-5."""
    import torch
    from dhr_amd import gip_scores as GS
    from dhr_amd import lexical_train as LT
    gen = torch.Generator(device="cuda").manual_seed(29)
    V, dims, remove, n_q, n_pass = 4026, 64, 58, 3, 2
    sides = {}
    for side, B, L in (("q", n_q, 8), ("p", n_q * n_pass, 12)):
        lg = (torch.randn((B, L, V), generator=gen, device="cuda") * 2).half().requires_grad_(True)
        w = torch.randn((B, L - 1, 1), generator=gen, device="cuda").abs().half().requires_grad_(True)
        mask = (torch.arange(L - 1, device="cuda")[None] < torch.randint(2, L, (B, 1), generator=gen, device="cuda")).long()
        sides[side] = (lg, w, mask)

    def step(head):
        res = {}
        for side, (lg, w, mask) in sides.items():
            lg.grad = w.grad = None
            reps, tok = head(lg, w, mask)
            reps.retain_grad()
            res[side] = (reps, tok)
        scores = GS.listwise_gip_scores(res["q"][0], res["p"][0], n_q, dims, remove)
        labels = torch.nn.functional.one_hot(torch.arange(n_q, device="cuda") * n_pass, num_classes=scores.size(1)).float()
        loss = torch.nn.KLDivLoss(reduction="batchmean")(torch.nn.functional.log_softmax(scores, dim=-1), labels)
        loss.backward()
        return float(loss.detach()), {s: (res[s][0].grad.clone(), res[s][1], sides[s][0].grad.clone(), sides[s][1].grad.clone()) for s in sides}

    loss_new, new = step(lambda lg, w, mask: LT.lexical_reps(lg, w, mask, skip_tokens=1, return_tokens=True))
    loss_old, old = step(lambda lg, w, mask: _eager(lg, w, mask))
    print(f"composed step: loss {loss_new:.7f} (this head) / {loss_old:.7f} (eager head)")
    assert abs(loss_new - loss_old) <= 1e-5 * abs(loss_old)
    for side, (lg, w, mask) in sides.items():
        xn, wn, mn = _np(lg)[:, 1:], _np(w)[..., 0], mask.cpu().numpy()
        p, d, r, a, near, c = forward64(xn, wn, mn)
        for tag, (G, tok, gx, gw) in (("this head", new[side]), ("eager head", old[side])):
            assert G.any() and not gx[:, 0].any()
            check_routing(tok.cpu().numpy(), a, near, c, f"composed {side} {tag}")
            _check_grads(f"composed {side} {tag}", p, d, wn, mn, _np(G), tok.cpu().numpy(), _np(gx)[:, 1:], _np(gw)[..., 0], True, True)
        print(f"composed {side}: max |dL/dlogits (this head) - (eager head)| = {float((new[side][2].float() - old[side][2].float()).abs().max()):.3e}, "
              f"max |dL/dlogits| = {float(old[side][2].float().abs().max()):.3e}")


@pytest.mark.gpu
def test_memory_of_forward_and_backward():
    """B = 32, L = 64 (T = 63), V = 30522, fp16: with N the bytes of the logits, the forward's peak above the live inputs stays below N / 2 (it
    holds 6 bytes per (b, v) and 20 per (b, t)) and the backward's peak above what is live before it below N (the gradient it returns) + N / 2.
    The eager composition on the same shape is measured and printed: it keeps fp32 [B, T, V] tensors and meets neither limit."""
    import torch
    from dhr_amd import lexical_train as LT
    B, L, V = 32, 64, 30522
    gen = torch.Generator(device="cuda").manual_seed(31)
    lg = torch.randn((B, L, V), generator=gen, device="cuda", dtype=torch.float16).requires_grad_(True)
    w = torch.randn((B, L - 1, 1), generator=gen, device="cuda", dtype=torch.float16).requires_grad_(True)
    mask = torch.ones((B, L - 1), dtype=torch.int64, device="cuda")
    G = torch.randn((B, V), generator=gen, device="cuda")
    N = lg.numel() * lg.element_size()
    LT.lexical_reps(lg, w, mask, skip_tokens=1).backward(G)                        # warm-up: the library is loaded, kernels are resident
    peaks = {}
    for name, head in (("library", lambda: LT.lexical_reps(lg, w, mask, skip_tokens=1)), ("eager", lambda: _eager(lg, w, mask)[0])):
        lg.grad = w.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        reps = head()
        torch.cuda.synchronize()
        fwd = torch.cuda.max_memory_allocated() - before
        mid = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        reps.backward(G)
        torch.cuda.synchronize()
        bwd = torch.cuda.max_memory_allocated() - mid
        peaks[name] = (fwd, bwd)
        del reps
    for name, (fwd, bwd) in peaks.items():
        print(f"memory ({name}): forward peak {fwd / N:.3f} N, backward peak {bwd / N:.3f} N  (N = {N} B of logits; limits 0.5 N and 1.5 N)")
    fwd, bwd = peaks["library"]
    assert fwd < N / 2 and fwd <= 0.05 * N
    assert bwd < N + N / 2
    assert peaks["eager"][0] >= 4 * N                                             # what makes the limits discriminating


@pytest.mark.gpu
def test_timing_against_the_eager_composition():
    """Forward + backward at the shapes of the reference's training recipe (24 queries x 8 passages per device, p_max_len 150, q_max_len 32,
    V = 30522, fp16 logits): device events, a warm-up, the median of 7, the two sides alternating.  Asserts only that this path is not slower
    than the eager composition at the passage shape."""
    import torch
    from dhr_amd import lexical_train as LT
    V = 30522
    ratios = {}
    for side, B, L in (("passages", 192, 150), ("queries", 24, 32)):
        lg = torch.randn((B, L, V), device="cuda", dtype=torch.float16).requires_grad_(True)
        w = torch.randn((B, L - 1, 1), device="cuda", dtype=torch.float16).requires_grad_(True)
        mask = torch.ones((B, L - 1), dtype=torch.int64, device="cuda")
        G = torch.randn((B, V), device="cuda")

        def run(head):
            lg.grad = w.grad = None
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            reps = head()
            e[1].record()
            reps.backward(G)
            e[2].record()
            torch.cuda.synchronize()
            return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])

        heads = {"library": lambda: LT.lexical_reps(lg, w, mask, skip_tokens=1), "eager": lambda: _eager(lg, w, mask)[0]}
        times = {k: [] for k in heads}
        for it in range(9):
            for name, head in heads.items():
                t = run(head)
                if it >= 2:
                    times[name].append(t)
        med = {k: (float(np.median([a for a, _ in v])), float(np.median([b for _, b in v]))) for k, v in times.items()}
        elems = B * (L - 1) * V
        lf, lb = med["library"]
        ef, eb = med["eager"]
        ratios[side] = (ef + eb) / (lf + lb)
        print(f"lexical head fwd+bwd {side} B={B} L={L} V={V} fp16: library {lf:.3f} + {lb:.3f} ms, eager torch {ef:.3f} + {eb:.3f} ms, "
              f"{ratios[side]:.2f}x; library backward moves {4 * elems / lb / 1e9:.2f} TB/s of logits read + gradient written")
        lg.grad = w.grad = None
        del lg, w, G
        torch.cuda.empty_cache()
    assert ratios["passages"] >= 1.0
