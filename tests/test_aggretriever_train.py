"""The Aggretriever training ops (dhr_amd/aggretriever_train.py on dhr_aggregate_train / dhr_aggregate_backward / dhr_term_weight_head /
dhr_term_weight_head_backward, dhr_amd/csrc/aggretriever_train.hip) against the reference's own code under autograd
(tests/golden/aggretriever_train_golden.npz, made by tests/golden/make_golden_aggretriever_train.py), a float64 / numpy restatement kept here
that shares no code with the library, and the eager torch composition of the reference's lines on the same device.

Both ops are selections: every output and every gradient entry is an input value, its negation or zero.  So there is no tolerance anywhere in
this file: values are compared with == (signed zeros may differ in the forward), routes and gradients with array_equal.  The eager
composition on the device is comparable only where its max has one winner (torch.max on a GPU does not promise the first index): the dense
random cases have no ties, and in the sparse chain the weights are pairwise distinct and non-zero, which makes the outputs and dL/dw unique
(a tie among zeros routes to a column no token won, which reaches no weight either way); dL/dreps of the sparse chain is checked against the
restatement instead.

CPU part (-m "not gpu"): the fixture against the restatement; the entry points' declarations and statuses; the wrappers' errors.  GPU part:
goldens, bit-identity with dhr_amd.lexical.aggregate, strided views, the eager composition, repeated ids, out-of-range ids, a composed step
with both heads, memory, the library calls."""
import os

import numpy as np
import pytest

from dhr_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "aggretriever_train_golden.npz")
V = 30522
NEW_SYMBOLS = ("dhr_aggregate_train", "dhr_aggregate_backward", "dhr_term_weight_head", "dhr_term_weight_head_backward")
AGGS = ((640, True), (768, True), (128, True), (640, False), (768, False))
CHAIN_REMOVE = {(640, True): -198, (768, True): -198, (128, True): 58, (640, False): 442, (768, False): 570}      # the issue's table
ALONE = (("dense", AGGS), ("v186b1", ((16, True),)), ("v186b5", ((16, True),)), ("v57b1", ((9, False),)), ("v57b5", ((9, False),)))


# ------------------------------------------------------------------------------------------ float64 / numpy restatement
def remove_of(width):
    """cal_remove_dim: the reference takes it from BERT's 30522 ids whatever the vocabulary of the tensor"""
    r = 30522 % width
    return r - width if r > 1000 else r


def agg_truth(x, dims, full, G=None):
    """x [B, vocab] -> dict: out [B, dims], route [B, dims], col [B, dims] (the routed vocabulary column, >= vocab in the padding),
    dreps [B, vocab] for the upstream G [B, dims]"""
    x = np.asarray(x, np.float64)
    B, vocab = x.shape
    W = 2 * dims if full else dims
    remove = remove_of(W)
    base = max(remove, 0)
    body = x[:, base:] if remove >= 0 else np.concatenate([x, np.zeros((B, -remove))], 1)
    view = body.reshape(B, -1, W)
    m, g = view.max(1), view.argmax(1)                                # numpy's argmax returns the first maximum
    j = np.arange(dims)[None, :]
    if full:
        pos, neg = m[:, 0::2], m[:, 1::2]
        s = (pos <= neg).astype(np.int64)
        out = np.where(s == 1, -neg, pos)
        grp = np.where(s == 1, g[:, 1::2], g[:, 0::2])
        route, col, sign = 2 * grp + s, base + grp * W + 2 * j + s, 1.0 - 2.0 * s
    else:
        out, route, col, sign = m, g, base + g * W + j, np.ones((B, dims))
    res = dict(out=out, route=route, col=col, remove=remove)
    if G is not None:
        d = np.zeros((B, vocab))
        for b in range(B):
            ok = col[b] < vocab                                        # a winner in the padding has no column
            d[b, col[b][ok]] = (sign[b] * np.asarray(G, np.float64)[b])[ok]
        res["dreps"] = d
    return res


def head_truth(ids, w, vocab, skip, G=None):
    """ids [B, L], w [B, L - skip] -> dict: reps [B, vocab], tok [B, vocab], dw [B, L - skip] for the upstream G [B, vocab]"""
    ids, w = np.asarray(ids, np.int64), np.asarray(w, np.float64)
    B, T = w.shape
    reps, tok = np.zeros((B, vocab)), -np.ones((B, vocab), np.int64)
    for b in range(B):
        for t in range(T):
            v = int(ids[b, skip + t])
            if 0 <= v < vocab and w[b, t] > reps[b, v]:                # strictly larger: the zero and the earlier token keep a tie
                reps[b, v], tok[b, v] = w[b, t], t
    res = dict(reps=reps, tok=tok)
    if G is not None:
        dw = np.zeros((B, T))
        for b in range(B):
            for t in range(T):
                v = int(ids[b, skip + t])
                if 0 <= v < vocab and tok[b, v] == t:
                    dw[b, t] = np.asarray(G, np.float64)[b, v]
        res["dw"] = dw
    return res


def key(dims, full):
    return "{}{}".format(dims, "f" if full else "s")


def _golden():
    return np.load(GOLDEN)


# ------------------------------------------------------------------------------------------ CPU part
def test_fixture_matches_restatement():
    z = _golden()
    assert os.path.getsize(GOLDEN) < 500_000
    for name in ("chain", "neg"):
        ids, w, reps = z[name + "_ids"], z[name + "_w"], z[name + "_reps"]
        assert ids.shape == (3, 9) and w.shape == (3, 8) and reps.shape == (3, V) and w.dtype == np.float32 and not (w == 0).any()
        assert np.array_equal(reps, head_truth(ids, w, V, 1)["reps"])
        for dims, full in AGGS:
            k = name + "_" + key(dims, full)
            t = agg_truth(reps, dims, full, z[k + "_G"])
            assert t["remove"] == CHAIN_REMOVE[(dims, full)]
            G = z[k + "_G"]
            assert (G == 0).any() and (G < 0).any() and (G > 0).any()
            assert np.array_equal(z[k + "_out"], t["out"]), k
            assert np.array_equal(z[k + "_dreps"], t["dreps"]), k
            assert np.array_equal(z[k + "_dw"], head_truth(ids, w, V, 1, z[k + "_dreps"])["dw"]), k
    # the designed cases do what they were designed for
    ids, w = z["chain_ids"], z["chain_w"]
    h = head_truth(ids, w, V, 1)
    assert ids[0, 1] == ids[0, 2] and 0 < w[0, 0] < w[0, 1] and h["tok"][0, 2000] == 1          # a repeat, the larger weight later
    assert ids[1, 1] == ids[1, 4] and w[1, 0] > w[1, 3] > 0 and h["tok"][1, 4000] == 0          # a repeat, the larger weight earlier
    assert (ids[:, -1] == 0).all() and (ids[2, 4:] == 0).all()                                  # trailing padding ids
    assert ids[0, 4] == 5 and ids[0, 5] == 441 and 441 < 442 and ids[1, 5] == 442               # ids inside / at the end of the removed columns
    assert z["chain_640s_dw"].any() and not z["chain_640s_dw"][0, 3:5].any() and not z["chain_640s_dreps"][:, :442].any()
    assert (z["neg_w"] < 0).all() and not z["neg_reps"].any() and not z["neg_640f_dw"].any() and z["neg_640f_dreps"].any()
    for name, aggs in ALONE:
        x = z[name + "_x4"].astype(np.float64) / 4
        for dims, full in aggs:
            k = name + "_" + key(dims, full)
            t = agg_truth(x, dims, full, z[k + "_G"])
            assert np.array_equal(z[k + "_out"], t["out"]) and np.array_equal(z[k + "_dreps"], t["dreps"]), k
    x = z["dense_x4"].astype(np.float64) / 4
    t = agg_truth(x, 640, True, z["dense_640f_G"])
    assert x[0, 3 * 1280 + 10] == x[0, 7 * 1280 + 10] == x[0, 10::1280].max() and t["route"][0, 5] == 2 * 3        # an equal maximum in two groups
    assert t["route"][0, 20] == 2 * 2 + 1 and t["out"][0, 20] == -9.5 and x[0, 5 * 1280 + 40] == 9.5              # pos == neg, non-zero
    assert t["route"][0, 550] == 2 * 23 + 1 and t["col"][0, 550] >= V and t["out"][0, 550] == 0                   # the zero padding wins
    assert z["dense_640f_G"][0, 550] != 0 and (x[0, 1100::1280] < 0).all() and (x[0, 1101::1280] < 0).all()
    assert z["v186b5_x4"].shape == (5, 186) and remove_of(32) == 26 == 186 % 32 and z["v57b1_x4"].shape == (1, 57) and remove_of(9) == 3 == 57 % 9
    # quantised values in a handful of groups tie often: the first group must have been taken
    ties = 0
    for name, remove, width in (("v186b5", 26, 32), ("v57b5", 3, 9)):
        top = np.sort(z[name + "_x4"][:, remove:].reshape(5, -1, width), 1)
        ties += int((top[:, -1] == top[:, -2]).sum())
    assert ties >= 3


def test_new_symbols_are_declared_everywhere():
    header = open(os.path.join(HERE, "..", "include", "dhr_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and name + "(" in header
        getattr(lib, name)
    vmap = open(os.path.join(HERE, "..", "dhr_amd", "csrc", "libdhr.map")).read()
    assert "dhr_*;" in vmap and "local:" in vmap
    assert lib.dhr_version() == 105


_A = dict(x=np.zeros((2, 186), np.float32), out=np.zeros((2, 16), np.float32), route=np.zeros((2, 16), np.int16), g=np.zeros((2, 16), np.float32),
          dx=np.zeros((2, 186), np.float32), ids=np.zeros((2, 5), np.int64), w=np.ones((2, 4), np.float32), reps=np.zeros((2, 64), np.float32),
          tok=np.zeros((2, 64), np.int16), gr=np.zeros((2, 64), np.float32), dw=np.zeros((2, 4), np.float32))
_P = {k: v.ctypes.data for k, v in _A.items()}


def _call(fn, defaults, kw):
    a = dict(defaults)
    assert set(kw) <= set(a), kw
    a.update(kw)
    return fn(*a.values())


def test_entry_points_return_statuses():
    """HOST arrays throughout: a valid call must come back as DHR_ERR_UNSUPPORTED (training tensors live on the device) and every invalid one
    as DHR_ERR_INVALID before that, so nothing here touches a device."""
    lib = _lib.load()
    H = _lib.MEM_HOST
    agg_f = dict(device=0, mem_kind=H, lexical=_P["x"], value_dtype=_lib.VAL_F32, ld=186, batch=2, vocab=186, dims=16, remove=26, full=1, out=_P["out"],
                 out_dtype=_lib.VAL_F32, ld_out=16, route=_P["route"], ld_route=16, stream=None)
    agg_b = dict(device=0, mem_kind=H, grad_out=_P["g"], grad_dtype=_lib.VAL_F32, ld_grad_out=16, route=_P["route"], ld_route=16, batch=2, vocab=186,
                 dims=16, remove=26, full=1, dx=_P["dx"], ld_grad=186, stream=None)
    tw_f = dict(device=0, mem_kind=H, ids=_P["ids"], id_bytes=8, ld_ids=5, w=_P["w"], value_dtype=_lib.VAL_F32, ld_w=4, batch=2, n_tokens=4, skip=1,
                vocab=64, reps=_P["reps"], ld_reps=64, tok=_P["tok"], ld_tok=64, stream=None)
    tw_b = dict(device=0, mem_kind=H, ids=_P["ids"], id_bytes=8, ld_ids=5, batch=2, n_tokens=4, skip=1, vocab=64, grad_reps=_P["gr"], ld_grad_reps=64,
                tok=_P["tok"], ld_tok=64, dw=_P["dw"], grad_dtype=_lib.VAL_F32, ld_dw=4, stream=None)
    fns = {"af": (lib.dhr_aggregate_train, agg_f), "ab": (lib.dhr_aggregate_backward, agg_b), "tf": (lib.dhr_term_weight_head, tw_f),
           "tb": (lib.dhr_term_weight_head_backward, tw_b)}
    run = lambda which, **kw: _call(*fns[which], kw)      # noqa: E731
    for which in fns:                                     # valid but on the host
        assert run(which) == _lib.ERR_UNSUPPORTED and b"DHR_MEM_DEVICE" in lib.dhr_last_error(), which
    invalid = {
        "af": [dict(lexical=None), dict(out=None), dict(batch=0), dict(batch=-1), dict(vocab=0), dict(value_dtype=5), dict(out_dtype=-1), dict(ld=185),
               dict(ld_out=15), dict(ld_route=15), dict(mem_kind=7), dict(dims=0), dict(dims=15, remove=26, ld_out=16), dict(remove=25), dict(remove=-6, full=0),
               dict(remove=186)],
        "ab": [dict(grad_out=None), dict(route=None), dict(dx=None), dict(batch=0), dict(vocab=-186), dict(grad_dtype=2), dict(ld_grad=185), dict(ld_grad_out=15),
               dict(ld_route=0), dict(mem_kind=-1), dict(dims=0), dict(remove=27), dict(remove=-6, full=0)],
        "tf": [dict(ids=None), dict(w=None), dict(reps=None), dict(tok=None), dict(batch=0), dict(n_tokens=0), dict(vocab=0), dict(skip=-1), dict(id_bytes=2),
               dict(id_bytes=0), dict(value_dtype=3), dict(ld_ids=4), dict(ld_w=3), dict(ld_reps=63), dict(ld_tok=63), dict(mem_kind=2)],
        "tb": [dict(ids=None), dict(grad_reps=None), dict(tok=None), dict(dw=None), dict(batch=0), dict(n_tokens=-4), dict(vocab=0), dict(skip=-1),
               dict(id_bytes=16), dict(grad_dtype=-1), dict(ld_ids=4), dict(ld_grad_reps=63), dict(ld_tok=63), dict(ld_dw=3), dict(mem_kind=9)],
    }
    for which, cases in invalid.items():
        for kw in cases:
            assert run(which, **kw) == _lib.ERR_INVALID and lib.dhr_last_error(), (which, kw)
    assert run("af", remove=25) == _lib.ERR_INVALID and b"whole number of groups" in lib.dhr_last_error()
    assert run("ab", remove=27) == _lib.ERR_INVALID and b"whole number of groups" in lib.dhr_last_error()
    assert run("af", lexical=None) == _lib.ERR_INVALID and b"null pointer" in lib.dhr_last_error()
    assert run("tf", id_bytes=2) == _lib.ERR_INVALID and b"int32 or int64" in lib.dhr_last_error()
    # a NULL route is legal in the forward (nothing to differentiate): still only the host refusal
    assert run("af", route=None, ld_route=0) == _lib.ERR_UNSUPPORTED and b"DHR_MEM_DEVICE" in lib.dhr_last_error()
    # 16384 groups of one column: 2 * g + 1 no longer fits the route; 16383 pass that check
    for which in ("af", "ab"):
        big = dict(vocab=16384, dims=1, remove=0, full=0, ld=16384) if which == "af" else dict(vocab=16384, dims=1, remove=0, full=0, ld_grad=16384)
        assert run(which, **big) == _lib.ERR_UNSUPPORTED and b"16383" in lib.dhr_last_error(), which
        big.update(vocab=16383)
        assert run(which, **big) == _lib.ERR_UNSUPPORTED and b"DHR_MEM_DEVICE" in lib.dhr_last_error(), which
    for which in ("tf", "tb"):
        long = dict(n_tokens=32768, ld_ids=32769, ld_w=32768) if which == "tf" else dict(n_tokens=32768, ld_ids=32769, ld_dw=32768)
        assert run(which, **long) == _lib.ERR_UNSUPPORTED and b"32767" in lib.dhr_last_error(), which
        long = {k: v - 1 for k, v in long.items()}
        assert run(which, **long) == _lib.ERR_UNSUPPORTED and b"DHR_MEM_DEVICE" in lib.dhr_last_error(), which


def test_wrappers_raise_before_touching_the_library(monkeypatch):
    import torch
    from dhr_amd import aggretriever_train as AT

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    for make in (lambda *s: torch.zeros(*s), lambda *s: torch.zeros(*s, requires_grad=True)):
        with pytest.raises(ValueError, match="shape should be 2"):
            AT.aggregate(make(2, 3, V))
        with pytest.raises(ValueError, match="shape should be 2"):
            AT.aggregate(make(V))
        with pytest.raises(ValueError, match=r"cal_remove_dim\(1400\) = -278 is negative"):    # 30522 % 1400 = 1122 > 1000
            AT.aggregate(make(2, V), dims=1400, full=False)
        with pytest.raises(RuntimeError, match="0 elements"):
            AT.aggregate(make(0, 186), dims=16)
        with pytest.raises(RuntimeError, match="0 elements"):                                  # fewer columns than one group
            AT.aggregate(make(2, 20), dims=16)
        with pytest.raises(_lib.DhrError, match="must live on a GPU"):
            AT.aggregate(make(2, 186), dims=16)
        with pytest.raises(_lib.DhrError, match="must live on a GPU"):
            AT.aggregate(make(2, V))
        with pytest.raises(_lib.DhrError, match="must live on a GPU"):
            AT.term_weight_reps(torch.zeros((2, 5), dtype=torch.long), make(2, 4, 1))
    with pytest.raises(_lib.DhrError, match="torch tensor"):
        AT.aggregate(np.zeros((2, 186), np.float32), dims=16)
    with pytest.raises(_lib.DhrError, match="unsupported lexical reps dtype"):
        AT.aggregate(torch.zeros((2, 186), dtype=torch.float64), dims=16)
    with pytest.raises(_lib.DhrError, match="16383 groups"):
        AT.aggregate(torch.zeros((1, 16384)), dims=1, full=False)
    ids, w = torch.zeros((2, 5), dtype=torch.long), torch.zeros((2, 4))
    with pytest.raises(_lib.DhrError, match="torch tensors"):
        AT.term_weight_reps(ids.numpy(), w)
    with pytest.raises(_lib.DhrError, match="torch tensors"):
        AT.term_weight_reps(ids, w.numpy())
    with pytest.raises(ValueError, match="got 3 dimensions"):
        AT.term_weight_reps(ids[:, :, None], w)
    for bad in (torch.zeros((2, 5)), torch.zeros((2, 3)), torch.zeros((3, 4)), torch.zeros((2, 4, 2)), torch.zeros((2, 4, 1, 1)), torch.zeros(8)):
        with pytest.raises(ValueError, match=r"term_weights must be \[2, 4\] or \[2, 4, 1\]"):
            AT.term_weight_reps(ids, bad)
    with pytest.raises(ValueError, match="no tokens"):
        AT.term_weight_reps(ids, torch.zeros((2, 0)), skip_tokens=5)
    with pytest.raises(ValueError, match="skip_tokens must be >= 0"):
        AT.term_weight_reps(ids, w, skip_tokens=-1)
    with pytest.raises(ValueError, match="vocab must be > 0"):
        AT.term_weight_reps(ids, w, vocab=0)
    with pytest.raises(ValueError, match="more than 32767 tokens"):
        AT.term_weight_reps(torch.zeros((1, 32769), dtype=torch.long), torch.zeros((1, 32768)))
    with pytest.raises(_lib.DhrError, match="unsupported input_ids dtype"):
        AT.term_weight_reps(ids.to(torch.int16), w)
    with pytest.raises(_lib.DhrError, match="unsupported term_weights dtype"):
        AT.term_weight_reps(ids, w.double())


# ------------------------------------------------------------------------------------------ GPU part
def _np(t):
    return t.detach().float().cpu().numpy()


def _eager_aggregate(lexical_reps, dims, full):
    """tevatron/Aggretriever/utils.py:22-44, the same torch ops on whatever device the reps live on"""
    import torch
    batch_size = lexical_reps.shape[0]
    if full:
        remove_dims = remove_of(dims * 2)
        if remove_dims >= 0:
            lexical_reps = lexical_reps[:, remove_dims:].view(batch_size, -1, dims * 2)
        else:
            lexical_reps = torch.nn.functional.pad(lexical_reps, (0, -remove_dims), "constant", 0).view(batch_size, -1, dims * 2)
        tok_reps, _ = lexical_reps.max(1)
        pos, neg = tok_reps[:, 0:2 * dims:2], tok_reps[:, 1:2 * dims:2]
        return pos * (pos > neg) - neg * (pos <= neg)
    remove_dims = remove_of(dims)
    return lexical_reps[:, remove_dims:].view(batch_size, -1, dims).max(1)[0]


def _eager_head(input_ids, term_weights, vocab=V):
    """tevatron/Aggretriever/modeling.py:282-284: term_weights [B, L - 1, 1], the zero tensor has L rows"""
    import torch
    B, L = input_ids.shape
    reps = torch.zeros(B, L, vocab, dtype=term_weights.dtype, device=term_weights.device)
    reps = torch.scatter(reps, dim=-1, index=input_ids[:, 1:, None], src=term_weights)
    return reps.max(-2).values


def _bits(t):
    import torch
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


@pytest.mark.gpu
def test_goldens_on_gpu():
    import torch
    from dhr_amd import aggretriever_train as AT
    z = _golden()
    for name in ("chain", "neg"):
        ids, w_np = z[name + "_ids"], z[name + "_w"]
        h = head_truth(ids, w_np, V, 1)
        for id_dtype in (torch.int64, torch.int32):
            t_ids = torch.from_numpy(ids).to("cuda", id_dtype)
            for dims, full in AGGS:
                k = name + "_" + key(dims, full)
                w = torch.from_numpy(w_np).cuda()[..., None].requires_grad_(True)                     # [B, L - 1, 1] like the Linear's output
                reps, tok = AT.term_weight_reps(t_ids, w, return_tokens=True)
                reps.retain_grad()
                out, route = AT.aggregate(reps, dims, full, return_route=True)
                out.backward(torch.from_numpy(z[k + "_G"]).cuda())
                t = agg_truth(z[name + "_reps"], dims, full)
                assert reps.dtype == torch.float32 and tok.dtype == torch.int16 and route.dtype == torch.int16 and not tok.requires_grad
                assert (_np(reps) == z[name + "_reps"]).all() and np.array_equal(tok.cpu().numpy(), h["tok"]), k
                assert (_np(out) == z[k + "_out"]).all() and np.array_equal(route.cpu().numpy(), t["route"]), k
                assert np.array_equal(_np(reps.grad), z[k + "_dreps"]), k
                assert tuple(w.grad.shape) == tuple(w.shape) and np.array_equal(_np(w.grad)[..., 0], z[k + "_dw"]), k
    for name, aggs in ALONE:
        x4 = z[name + "_x4"]
        for dtype in (torch.float32, torch.float16):                                                # multiples of 0.25 below 16: exact in fp16
            for dims, full in aggs:
                k = name + "_" + key(dims, full)
                x = (torch.from_numpy(x4).to("cuda", dtype) / 4).requires_grad_(True)
                out, route = AT.aggregate(x, dims, full, return_route=True)
                out.backward(torch.from_numpy(z[k + "_G"]).to("cuda", dtype))
                t = agg_truth(x4 / 4.0, dims, full)
                assert out.dtype == dtype and x.grad.dtype == dtype
                assert (_np(out) == z[k + "_out"]).all() and np.array_equal(route.cpu().numpy(), t["route"]), (k, dtype)
                assert np.array_equal(_np(x.grad), z[k + "_dreps"]), (k, dtype)


@pytest.mark.gpu
def test_aggregate_forward_is_bit_identical_to_the_encoding_op_and_views_are_read_in_place():
    """seeded random [5, 30522] and [4, 186] reps, fp32 and fp16, contiguous and as the [:, :V] view of a V + 1 wide tensor (an odd fp16 row
    stride): the values carry the bits of dhr_amd.lexical.aggregate, and the gradient of the view equals that of its contiguous copy."""
    import torch
    from dhr_amd import aggretriever_train as AT
    from dhr_amd import lexical as LX
    gen = torch.Generator(device="cuda").manual_seed(41)
    for B, vocab, aggs in ((5, V, AGGS), (4, 186, ((16, True),)), (3, 57, ((9, False),))):
        for dtype in (torch.float32, torch.float16):
            wide = torch.randn((B, vocab + 1), generator=gen, device="cuda").to(dtype)
            wide[:, ::7] = 0                                                                       # exact zeros: ties with the padding and between groups
            wide[0, : vocab // 2] = -wide[0, : vocab // 2].abs()
            for dims, full in aggs:
                G = torch.randn((B, dims), generator=gen, device="cuda").to(dtype)
                want = LX.aggregate(wide[:, :vocab], dims, full=full)
                base = wide.clone().requires_grad_(True)
                view = base[:, :vocab]
                assert not view.is_contiguous()
                out_v, route_v = AT.aggregate(view, dims, full, return_route=True)
                out_v.backward(G)
                flat = wide[:, :vocab].contiguous().requires_grad_(True)
                out_c, route_c = AT.aggregate(flat, dims, full, return_route=True)
                out_c.backward(G)
                assert out_v.dtype == dtype and torch.equal(_bits(out_v.detach()), _bits(want)) and torch.equal(_bits(out_c.detach()), _bits(want))
                assert torch.equal(route_v, route_c)
                assert tuple(base.grad.shape) == (B, vocab + 1) and not base.grad[:, vocab].any()
                assert torch.equal(_bits(base.grad[:, :vocab].contiguous()), _bits(flat.grad))
                t = agg_truth(_np(flat), dims, full, _np(G))
                assert np.array_equal(route_c.cpu().numpy(), t["route"]) and np.array_equal(_np(flat.grad), t["dreps"])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("dims,full", [(1, True), (3, False)])
def test_aggregate_backward_of_rows_shorter_than_one_vector(dtype, dims, full):
    """vocab = 6 is below the 8 columns a thread of the backward owns, so the row takes the element-wise stores whatever its dtype (an fp32
    row is never misaligned otherwise): three groups of 2 signed columns / two groups of 3, multiples of 0.25, against the restatement."""
    import torch
    from dhr_amd import aggretriever_train as AT
    rng = np.random.default_rng(71)
    B, vocab = 3, 6
    assert remove_of(2 * dims if full else dims) == 0
    x4 = rng.integers(-12, 13, (B, vocab))
    x4[0, :2] = x4[0, 2:4]                                                                         # an equal maximum in two groups
    G4 = rng.integers(-8, 9, (B, dims))
    tdt = getattr(torch, dtype)
    x = (torch.from_numpy(x4).to("cuda", tdt) / 4).requires_grad_(True)
    out, route = AT.aggregate(x, dims, full, return_route=True)
    out.backward(torch.from_numpy(G4).to("cuda", tdt) / 4)
    t = agg_truth(x4 / 4.0, dims, full, G4 / 4.0)
    assert out.dtype == tdt and x.grad.dtype == tdt and tuple(x.grad.shape) == (B, vocab)
    assert (_np(out) == t["out"]).all() and np.array_equal(route.cpu().numpy(), t["route"])
    assert np.array_equal(_np(x.grad), t["dreps"]) and x.grad.any()


@pytest.mark.gpu
@pytest.mark.parametrize("id_dtype", ["int64", "int32"])
@pytest.mark.parametrize("w_dtype", ["float32", "float16"])
@pytest.mark.parametrize("vocab", [4100, 4101])
def test_term_weight_head_of_every_id_and_weight_dtype_on_even_and_odd_rows(id_dtype, w_dtype, vocab):
    """int64 / int32 ids with fp32 / fp16 weights; the rows of the int16 token tensor start at a multiple of 4 bytes (vocab even) or do not
    (vocab odd: the element-wise stores); the vocabulary spans two workgroups of columns.  Forward, tokens and dL/dw against the restatement."""
    import torch
    from dhr_amd import aggretriever_train as AT
    rng = np.random.default_rng(73)
    B, L = 3, 12
    ids = rng.integers(0, vocab, (B, L)).astype(np.int64)
    ids[0, 3] = ids[0, 7]                                                                          # a repeated id
    ids[1, 5], ids[2, 6] = vocab - 1, 4096                                                         # the last column, the first of the second block
    w_np = (rng.permutation(B * (L - 1)).reshape(B, L - 1) - 10).astype(np.float32) / 8          # distinct multiples of 1/8, some negative
    G = (rng.integers(-8, 9, (B, vocab)) / 4.0).astype(np.float32)
    truth = head_truth(ids, w_np, vocab, 1, G)
    w = torch.from_numpy(w_np).to("cuda", getattr(torch, w_dtype)).requires_grad_(True)
    reps, tok = AT.term_weight_reps(torch.from_numpy(ids).to("cuda", getattr(torch, id_dtype)), w, vocab=vocab, return_tokens=True)
    reps.backward(torch.from_numpy(G).cuda())
    assert reps.dtype == torch.float32 and tok.dtype == torch.int16 and tok.is_contiguous() and w.grad.dtype == w.dtype
    assert np.array_equal(_np(reps), truth["reps"]) and np.array_equal(tok.cpu().numpy(), truth["tok"])
    assert np.array_equal(_np(w.grad), truth["dw"]) and w.grad.any()


@pytest.mark.gpu
def test_eager_composition_on_the_device():
    import torch
    from dhr_amd import aggretriever_train as AT
    gen = torch.Generator(device="cuda").manual_seed(43)
    # dense fp32 reps: continuous values, no ties
    for B, vocab, aggs in ((5, V, AGGS), (4, 186, ((16, True),))):
        x = torch.randn((B, vocab), generator=gen, device="cuda")
        for dims, full in aggs:
            G = torch.randn((B, dims), generator=gen, device="cuda")
            a, b = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
            out = AT.aggregate(a, dims, full)
            ref = _eager_aggregate(b, dims, full)
            out.backward(G)
            ref.backward(G)
            assert torch.equal(out.detach(), ref.detach()) and torch.equal(a.grad, b.grad), (vocab, dims, full)
    # the sparse no-MLM chain, fp16 weights: pairwise distinct, none zero, half of them negative; ids repeat inside rows
    B, L = 4, 33
    T = L - 1
    ids = torch.randint(0, V, (B, L), generator=gen, device="cuda")
    ids[0, 5] = ids[0, 20]
    ids[1, 1:9] = ids[1, 9]
    ids[2, 20:] = 0
    ids[3, 1], ids[3, 2] = V - 1, 441
    w0 = (((torch.randperm(B * T, generator=gen, device="cuda").float() - B * T // 2 + 0.5) / 64).reshape(B, T, 1)).half()
    assert w0.unique().numel() == B * T and not (w0 == 0).any() and (w0 < 0).any() and (w0 > 0).any()
    for dims, full in AGGS:
        G = torch.randn((B, dims), generator=gen, device="cuda")
        wa, wb = w0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
        reps = AT.term_weight_reps(ids, wa)
        reps.retain_grad()
        out = AT.aggregate(reps, dims, full)
        reps_e = _eager_head(ids, wb)
        out_e = _eager_aggregate(reps_e, dims, full)
        out.backward(G)
        out_e.backward(G.half())
        assert reps.dtype == torch.float32 and reps_e.dtype == torch.float16                        # fp16 weights are widened exactly
        assert torch.equal(reps.detach(), reps_e.detach().float()) and torch.equal(out.detach(), out_e.detach().float()), (dims, full)
        assert wa.grad.dtype == torch.float16 and tuple(wa.grad.shape) == (B, T, 1)
        h = head_truth(ids.cpu().numpy(), _np(w0)[..., 0], V, 1)
        t = agg_truth(h["reps"], dims, full, _np(G))
        assert np.array_equal(_np(reps.grad), t["dreps"])
        dw = head_truth(ids.cpu().numpy(), _np(w0)[..., 0], V, 1, t["dreps"])["dw"]
        assert np.array_equal(_np(wa.grad)[..., 0], dw.astype(np.float16).astype(np.float64)), (dims, full)
        # the eager chain runs in fp16 throughout: it hands the weights G rounded to fp16, and so does this one
        assert torch.equal(wa.grad, wb.grad), (dims, full)


@pytest.mark.gpu
def test_repeated_ids_are_order_independent():
    """A row of 300 tokens all carrying one id and a row of 40 distinct ids repeated; weights from a small grid so that equal weights meet:
    two runs are bit-identical and equal the restatement (the largest weight, its first position)."""
    import torch
    from dhr_amd import aggretriever_train as AT
    rng = np.random.default_rng(47)
    L = 301
    ids = np.zeros((2, L), np.int64)
    ids[0, 1:] = 12345
    ids[1, 1:] = np.resize(rng.permutation(V)[:40], L - 1)
    w_np = (rng.integers(-8, 9, (2, L - 1)) / 4.0).astype(np.float32)
    G = (rng.integers(-8, 9, (2, V)) / 4.0).astype(np.float32)
    truth = head_truth(ids, w_np, V, 1, G)
    runs = []
    for id_dtype in (torch.int64, torch.int32, torch.int64):
        w = torch.from_numpy(w_np).cuda().requires_grad_(True)
        reps, tok = AT.term_weight_reps(torch.from_numpy(ids).to("cuda", id_dtype), w, return_tokens=True)
        reps.backward(torch.from_numpy(G).cuda())
        runs.append((reps.detach(), tok, w.grad))
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], r))
    assert np.array_equal(_np(runs[0][0]), truth["reps"]) and np.array_equal(runs[0][1].cpu().numpy(), truth["tok"])
    assert np.array_equal(_np(runs[0][2]), truth["dw"]) and tuple(runs[0][2].shape) == (2, L - 1)
    assert int((truth["tok"] >= 0).sum()) == 1 + 40 and (w_np[0] == w_np[0].max()).sum() > 1


@pytest.mark.gpu
def test_ids_outside_the_vocabulary_are_ignored():
    import torch
    from dhr_amd import aggretriever_train as AT
    rng = np.random.default_rng(53)
    B, L, vocab = 3, 17, 5000                                                                    # vocab spans two workgroups of columns
    ids = rng.integers(0, vocab, (B, L)).astype(np.int64)
    w_np = rng.permutation(B * (L - 1)).reshape(B, L - 1).astype(np.float32) + 1
    G = rng.standard_normal((B, vocab)).astype(np.float32)
    clean = head_truth(ids, w_np, vocab, 1, G)
    bad = ids.copy()
    spots = ((0, 3, -1), (0, 4, vocab), (0, 5, vocab + 1), (1, 1, 2 ** 31 - 1), (1, 16, -5), (2, 8, vocab + 4095), (2, 9, 4096 * 2), (2, 12, 8191))
    for b, l, v in spots:
        bad[b, l] = v
    for id_dtype, extra in ((torch.int64, ((2, 10, 2 ** 40 + 7), (2, 11, -2 ** 33))), (torch.int32, ((2, 10, -2 ** 31),))):
        cur = bad.copy()
        for b, l, v in extra:
            cur[b, l] = v
        gone = [(b, l) for b, l, _ in spots + extra]
        w = torch.from_numpy(w_np).cuda().requires_grad_(True)
        reps, tok = AT.term_weight_reps(torch.from_numpy(cur).to("cuda", id_dtype), w, vocab=vocab, return_tokens=True)
        reps.backward(torch.from_numpy(G).cuda())
        torch.cuda.synchronize()
        truth = head_truth(cur, w_np, vocab, 1, G)
        assert np.array_equal(_np(reps), truth["reps"]) and np.array_equal(tok.cpu().numpy(), truth["tok"]) and np.array_equal(_np(w.grad), truth["dw"])
        for b, l in gone:
            assert w.grad[b, l - 1] == 0
        # no entry of reps changes beyond the columns the replaced tokens had won
        lost = np.zeros((B, vocab), bool)
        for b, l in gone:
            lost[b, ids[b, l]] = True
        assert np.array_equal(_np(reps)[~lost], clean["reps"][~lost])


@pytest.mark.gpu
def test_composed_step_with_both_heads():
    """encoder stub -> lexical reps -> aggregate -> listwise scores (matmul) -> log_softmax -> KL against one-hot labels -> backward, once with
    the MLM head (lexical_train.lexical_reps) and once with the no-MLM head, each against the eager composition.  Through the new ops the
    step is exact: aggregate's output and dL/dreps equal the restatement on the step's own reps and upstream gradient.  The existing MLM head
    keeps the bound and the routing rule of tests/test_lexical_train.py under its own dL/dreps."""
    import torch
    from dhr_amd import aggretriever_train as AT
    from dhr_amd import lexical_train as LT
    from tests import test_lexical_train as TL
    gen = torch.Generator(device="cuda").manual_seed(59)
    vocab, dims, n_q, n_pass = 4026, 64, 3, 2                                                     # remove 58, 31 groups of 128

    def loss_of(q, p):
        scores = torch.matmul(q, p.transpose(0, 1)).view(n_q, -1)
        labels = torch.nn.functional.one_hot(torch.arange(n_q, device="cuda") * n_pass, num_classes=scores.size(1)).float()
        return torch.nn.KLDivLoss(reduction="batchmean")(torch.nn.functional.log_softmax(scores, dim=-1), labels)

    # --- the MLM head
    sides = {}
    for side, B, L in (("q", n_q, 8), ("p", n_q * n_pass, 12)):
        lg = (torch.randn((B, L, vocab), generator=gen, device="cuda") * 2).half().requires_grad_(True)
        w = torch.randn((B, L - 1, 1), generator=gen, device="cuda").abs().half().requires_grad_(True)
        mask = (torch.arange(L - 1, device="cuda")[None] < torch.randint(2, L, (B, 1), generator=gen, device="cuda")).long()
        sides[side] = (lg, w, mask)

    def step(head, agg):
        res = {}
        for side, (lg, w, mask) in sides.items():
            lg.grad = w.grad = None
            reps, tok = head(lg, w, mask)
            reps.retain_grad()
            out = agg(reps)
            out.retain_grad()
            res[side] = (reps, tok, out)
        loss = loss_of(res["q"][2] * 64, res["p"][2] * 64)                                          # (softmax reps are small: scaled so that the loss moves)
        loss.backward()
        return float(loss.detach()), {s: res[s] + (sides[s][0].grad.clone(), sides[s][1].grad.clone()) for s in sides}

    loss_new, new = step(lambda lg, w, m: LT.lexical_reps(lg, w, m, skip_tokens=1, return_tokens=True), lambda r: AT.aggregate(r, dims, True))
    loss_old, old = step(lambda lg, w, m: TL._eager(lg, w, m), lambda r: _eager_aggregate(r, dims, True))
    print(f"composed step (MLM head): loss {loss_new:.7f} (library) / {loss_old:.7f} (eager)")
    assert abs(loss_new - loss_old) <= 1e-5 * abs(loss_old)
    for side, (lg, w, mask) in sides.items():
        xn, wn, mn = _np(lg)[:, 1:], _np(w)[..., 0], mask.cpu().numpy()
        p, d, r, a, near, c = TL.forward64(xn, wn, mn)
        for tag, (reps, tok, out, gx, gw) in (("library", new[side]), ("eager", old[side])):
            t = agg_truth(_np(reps), dims, True, _np(out.grad))
            assert np.array_equal(_np(out), t["out"]) and np.array_equal(_np(reps.grad), t["dreps"]) and reps.grad.any(), (side, tag)
            TL.check_routing(tok.cpu().numpy(), a, near, c, f"composed {side} {tag}")
            TL._check_grads(f"composed {side} {tag}", p, d, wn, mn, _np(reps.grad), tok.cpu().numpy(), _np(gx)[:, 1:], _np(gw)[..., 0], True, True)

    # --- the no-MLM head: sparse reps, the whole step equals the eager one bit for bit
    heads = {}
    for side, B, L in (("q", n_q, 8), ("p", n_q * n_pass, 12)):
        ids = torch.randint(0, vocab, (B, L), generator=gen, device="cuda")
        ids[:, L - 2:] = 0
        ids[0, 2] = ids[0, 1]
        T = L - 1
        w = ((torch.randperm(B * T, generator=gen, device="cuda").float() - B * T // 4 + 0.5) / 8).reshape(B, T, 1)
        heads[side] = (ids, w)

    def sparse_step(head, agg):
        ws = {s: heads[s][1].clone().requires_grad_(True) for s in heads}
        outs = {s: agg(head(heads[s][0], ws[s])) for s in heads}
        loss = loss_of(outs["q"], outs["p"])
        loss.backward()
        return loss.detach(), outs, {s: ws[s].grad for s in ws}

    for full in (True, False):
        l_new, o_new, g_new = sparse_step(lambda i, w: AT.term_weight_reps(i, w, vocab=vocab), lambda r: AT.aggregate(r, dims, full))
        l_old, o_old, g_old = sparse_step(lambda i, w: _eager_head(i, w, vocab), lambda r: _eager_aggregate(r, dims, full))
        assert torch.equal(l_new, l_old) and all(torch.equal(o_new[s].detach(), o_old[s].detach()) for s in heads), full
        assert all(torch.equal(g_new[s], g_old[s]) and g_new[s].any() for s in heads), full


@pytest.mark.gpu
def test_memory_stays_far_below_the_scatter_tensor():
    """B = 8, L = 64, V = 30522, fp32 weights: the peak over forward + backward of aggregate(term_weight_reps(...)), beyond the inputs and the
    returned tensors, stays below the bytes of ONE [B, L, V] tensor in the weights' dtype (62.5 MB), which the reference allocates and autograd
    keeps.  The op's own buffers are about 16 bytes per (b, v), under 4 MB: the cap tests for the absence of the temporary."""
    import torch
    from dhr_amd import aggretriever_train as AT
    B, L = 8, 64
    gen = torch.Generator(device="cuda").manual_seed(61)
    ids = torch.randint(0, V, (B, L), generator=gen, device="cuda")
    w = torch.randn((B, L - 1, 1), generator=gen, device="cuda").requires_grad_(True)
    G = torch.randn((B, 640), generator=gen, device="cuda")
    AT.aggregate(AT.term_weight_reps(ids, w)).backward(G)                                         # warm-up: the library is loaded
    w.grad = None
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = AT.aggregate(AT.term_weight_reps(ids, w))
    out.backward(G)
    torch.cuda.synchronize()
    returned = out.numel() * out.element_size() + w.grad.numel() * w.grad.element_size()
    peak = torch.cuda.max_memory_allocated() - before - returned
    cap = B * L * V * 4
    print(f"memory: peak beyond inputs and returned tensors {peak / 2 ** 20:.2f} MiB; one [B, L, V] fp32 tensor {cap / 2 ** 20:.2f} MiB")
    assert 0 < peak < cap


class _Spy:
    """the loaded library with the four entry points recorded"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in NEW_SYMBOLS:
            return fn

        def recorded(*args):
            self.calls.append((name, args))
            return fn(*args)
        return recorded


@pytest.mark.gpu
def test_one_library_call_per_op_and_direction(monkeypatch):
    import torch
    from dhr_amd import aggretriever_train as AT
    gen = torch.Generator(device="cuda").manual_seed(67)
    B, L = 3, 12
    ids = torch.randint(0, V, (B, L), generator=gen, device="cuda")
    w = torch.randn((B, L - 1), generator=gen, device="cuda").requires_grad_(True)
    wide = torch.randn((B, V + 2), generator=gen, device="cuda").requires_grad_(True)
    spy = _Spy(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: spy)
    out = AT.aggregate(AT.term_weight_reps(ids, w))
    assert [c[0] for c in spy.calls] == ["dhr_term_weight_head", "dhr_aggregate_train"]
    # (device, mem_kind, input_ids, id_bytes, ld_ids, term_weights, value_dtype, ld_weights, batch, n_tokens, skip_tokens, vocab, ...)
    assert spy.calls[0][1][1:12] == (_lib.MEM_DEVICE, ids.data_ptr(), 8, L, w.data_ptr(), _lib.VAL_F32, L - 1, B, L - 1, 1, V)
    out.backward(torch.ones_like(out))
    assert [c[0] for c in spy.calls[2:]] == ["dhr_aggregate_backward", "dhr_term_weight_head_backward"] and w.grad is not None
    # a strided view is read in place: the view's own pointer and row stride reach the library
    spy.calls.clear()
    view = wide[:, 1:V + 1]
    AT.aggregate(view).sum().backward()
    assert [c[0] for c in spy.calls] == ["dhr_aggregate_train", "dhr_aggregate_backward"]
    assert spy.calls[0][1][2] == view.data_ptr() and spy.calls[0][1][4] == V + 2 and not wide.grad[:, 0].any() and not wide.grad[:, V + 1].any()
    # nothing requires a gradient: the forwards only, and no graph
    spy.calls.clear()
    out = AT.aggregate(AT.term_weight_reps(ids, w.detach()))
    with torch.no_grad():
        out2 = AT.aggregate(AT.term_weight_reps(ids, w))
    assert [c[0] for c in spy.calls] == ["dhr_term_weight_head", "dhr_aggregate_train"] * 2
    assert not out.requires_grad and not out2.requires_grad and torch.equal(out, out2)
