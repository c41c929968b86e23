"""Differentiable gated-inner-product scores (dhr_amd/gip_scores.py on dhr_gip_scores / dhr_gip_scores_backward / dhr_densify_backward).

Truth is the float64 restatement below: densify with a first-wins argmax, an einsum over the match mask, gradients written out by hand (no
autograd).  The tolerance is derived, not measured: a result that is a sum of n products may be off by (n + 2) * 2^-24 * sum|terms|, evaluated
in float64 per entry, with n = dims for a score and n = the number of passages (queries) summed over for a query (passage) gradient; plus
2^-11 * |truth| where the output is fp16.  There is no absolute term: where every term is zero the result must be exactly zero, so the
sparsity pattern of the [B, V] gradients is checked by the same rule.

CPU part (-m "not gpu"): the golden fixture (the reference's own methods, tests/golden/make_golden_gip_scores.py) against the restatement;
statuses of the three entry points; the wrappers' errors.  GPU part: goldens, seeded random cases, bit-identity, memory, a timing printout."""
import os

import numpy as np
import pytest

from dhr_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gip_scores_golden.npz")
U32, U16 = 2.0 ** -24, 2.0 ** -11
MODES = ("list", "pair", "one")


# ------------------------------------------------------------------------------------------ float64 restatement
def densify64(reps, dims, remove):
    """-> (values float64 [B, dims], first group attaining them [B, dims])"""
    x = np.asarray(reps, np.float64)[:, remove:]
    x = x.reshape(x.shape[0], -1, dims)
    idx = x.argmax(1)                                            # numpy's argmax returns the first maximum
    return np.take_along_axis(x, idx[:, None, :], 1)[:, 0, :], idx


def truth_scores(qv, qi, pv, pi, G, pairs):
    """Densified float64 arrays, G [n_q, n_p] (zero outside `pairs`), pairs bool [n_q, n_p]: the (query, passage) pairs that are scored.
    -> (S, bound_S, dqv, bound_dqv, dpv, bound_dpv) with S [n_q, n_p]."""
    dims = qv.shape[1]
    match = (qi[:, None, :] == pi[None, :, :]) & pairs[:, :, None]
    terms = match * qv[:, None, :] * pv[None, :, :]
    S, bS = terms.sum(-1), (dims + 2) * U32 * np.abs(terms).sum(-1)
    tq = G[:, :, None] * match * pv[None, :, :]
    tp = G[:, :, None] * match * qv[:, None, :]
    n_for_q, n_for_p = int(pairs.sum(1).max()), int(pairs.sum(0).max())
    return (S, bS, tq.sum(1), (n_for_q + 2) * U32 * np.abs(tq).sum(1), tp.sum(0), (n_for_p + 2) * U32 * np.abs(tp).sum(0))


def scatter(dval, idx, vocab, dims, remove):
    """the gradient of densify: dval[b][j] at column remove + idx[b][j] * dims + j, zero elsewhere"""
    out = np.zeros((dval.shape[0], vocab), np.float64)
    cols = remove + idx * dims + np.arange(dims)[None, :]
    np.put_along_axis(out, cols, dval, 1)
    return out


def pairs_of(mode, n_q, n_p):
    """list: all pairs; pair: passage row b * n + j belongs to query b; one: row i with row i (one row on a side broadcasts)"""
    if mode == "list" or (mode == "one" and n_q != n_p):
        return np.ones((n_q, n_p), bool)
    n = n_p // n_q
    return (np.arange(n_p)[None, :] // n) == np.arange(n_q)[:, None]


def truth_reps(q, p, dims, remove, mode, G_ref):
    """[B, V] reps and G in the shape the reference returns -> dict of float64 truths and bounds, scores in the reference's shape."""
    qv, qi = densify64(q, dims, remove)
    pv, pi = densify64(p, dims, remove)
    n_q, n_p = qv.shape[0], pv.shape[0]
    pairs = pairs_of(mode, n_q, n_p)
    G = np.zeros((n_q, n_p))
    G[pairs] = np.asarray(G_ref, np.float64).reshape(-1)
    S, bS, dq, bq, dp, bp = truth_scores(qv, qi, pv, pi, G, pairs)
    shape = np.shape(G_ref)
    return dict(scores=S[pairs].reshape(shape), scores_bound=bS[pairs].reshape(shape),
                gq=scatter(dq, qi, q.shape[1], dims, remove), gq_bound=scatter(bq, qi, q.shape[1], dims, remove),
                gp=scatter(dp, pi, p.shape[1], dims, remove), gp_bound=scatter(bp, pi, p.shape[1], dims, remove), qi=qi, pi=pi)


def ref_shape(mode, n_q, n_p):
    """what the reference's squeeze leaves"""
    if mode == "one":
        return (max(n_q, n_p),)
    full = (n_q, 1, n_p if mode == "list" else n_p // n_q)
    return tuple(d for d in full if d != 1)


def assert_within(got, truth, bound, what, fp16=False):
    got = np.asarray(got.astype(np.float64) if isinstance(got, np.ndarray) else got, np.float64)
    assert got.shape == truth.shape, (what, got.shape, truth.shape)
    tol = bound + (U16 * np.abs(truth) if fp16 else 0.0)
    err = np.abs(got - truth)
    bad = err > tol
    worst = float((err / np.where(tol > 0, tol, 1.0))[tol > 0].max()) if (tol > 0).any() else 0.0
    print(f"{what}: max error / bound = {worst:.4f}, entries with a zero bound that are not zero: {int((err[tol == 0] != 0).sum())}")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} entries outside the bound (worst error / bound {worst:.3f})"


def golden_cases():
    z = np.load(GOLDEN)
    for name in z["names"]:
        dims, remove, bsz, n = (int(v) for v in z[name + "_geom"])
        for mode in MODES:
            p = z[name + "_p"] if mode != "one" else np.ascontiguousarray(z[name + "_p"][::n])
            yield f"{name}_{mode}", z, z[name + "_q"], p, dims, remove, bsz, n, mode


# ------------------------------------------------------------------------------------------ CPU part
def test_fixture_matches_float64_restatement():
    seen = 0
    for key, z, q, p, dims, remove, bsz, n, mode in golden_cases():
        G = z[key + "_G"]
        t = truth_reps(q, p, dims, remove, mode, G)
        assert z[key + "_scores"].shape == ref_shape(mode, q.shape[0], p.shape[0]), key
        assert_within(z[key + "_scores"], t["scores"], t["scores_bound"], key + " scores")
        assert_within(z[key + "_gq"], t["gq"], t["gq_bound"], key + " dL/dq_reps")
        assert_within(z[key + "_gp"], t["gp"], t["gp_bound"], key + " dL/dp_reps")
        assert not z[key + "_gq"][:, :remove].any() and not z[key + "_gp"][:, :remove].any()
        seen += 1
    assert seen == 18
    # the designed cases do what they were designed for
    t = truth_reps(z["ties_q"], z["ties_p"], 8, 570, "list", z["ties_list_G"])
    assert t["qi"][0, 1] == 0 and t["pi"][0, 1] == 1 and t["pi"][1, 1] == 2          # equal maxima: the first group
    assert not t["qi"][2].any() and not t["pi"][5].any()                             # all-zero rows sit at group 0 ...
    assert z["ties_list_gq"][2, 570:578].any() and not z["ties_list_gq"][2, 578:].any()   # ... and take their gradient at columns 570 .. 577
    t = truth_reps(z["wide_q"], z["wide_p"], 8, 570, "list", z["wide_list_G"])
    assert t["qi"].max() == 299 and t["pi"].max() == 299
    assert z["bsz1_list_scores"].shape == (5,) and z["n1_pair_scores"].shape == (4,) and z["prod_q"].shape == (3, 30522)
    kinds = [e.split(" | ")[1] for e in z["errors"]]
    assert kinds == ["RuntimeError"] * 5 + ["ValueError"] * 3


def _args(**kw):
    """valid host arguments of dhr_gip_scores / _backward (2 queries x 4 passages, 8 dims), with overrides"""
    a = dict(device=0, mem_kind=_lib.MEM_HOST, qv=_A["qv"].ctypes.data, ld_qv=8, qi=_A["qi"].ctypes.data, ld_qi=8, n_q=2, pv=_A["pv"].ctypes.data, ld_pv=8,
             pi=_A["pi"].ctypes.data, ld_pi=8, n_p=4, dims=8, value_dtype=_lib.VAL_F32, index_dtype=_lib.IDX_U8, group=0)
    a.update(kw)
    return list(a.values())


_A = dict(qv=np.ones((2, 8), np.float32), qi=np.zeros((2, 8), np.uint8), pv=np.ones((4, 8), np.float32), pi=np.zeros((4, 8), np.uint8),
          out=np.zeros((2, 4), np.float32), g=np.ones((2, 4), np.float32), dq=np.zeros((2, 8), np.float32), dp=np.zeros((4, 8), np.float32),
          dv=np.ones((2, 8), np.float32), idx=np.zeros((2, 8), np.uint8), grad=np.zeros((2, 42), np.float32))


def test_entry_points_return_statuses():
    import torch
    lib = _lib.load()
    for name in ("dhr_gip_scores", "dhr_gip_scores_backward", "dhr_densify_backward", "dhr_gip_scores_workspace"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    out, g, dq, dp = (_A[k].ctypes.data for k in ("out", "g", "dq", "dp"))

    def fwd(out=out, ld_out=4, ws_bytes=0, **kw):
        return lib.dhr_gip_scores(*_args(**kw), out, ld_out, None, ws_bytes, None)

    def bwd(g=g, ld_g=4, dq=dq, ld_dq=8, dp=dp, ld_dp=8, **kw):
        return lib.dhr_gip_scores_backward(*_args(**kw), g, ld_g, dq, ld_dq, dp, ld_dp, None)

    def dbw(dv=_A["dv"].ctypes.data, ld_dv=8, idx=_A["idx"].ctypes.data, idx_dtype=_lib.IDX_U8, ld_idx=8, batch=2, vocab=42, remove=10, dims=8,
            grad=_A["grad"].ctypes.data, grad_dtype=_lib.VAL_F32, ld_grad=42, mem_kind=_lib.MEM_HOST):
        return lib.dhr_densify_backward(0, mem_kind, dv, ld_dv, idx, idx_dtype, ld_idx, batch, vocab, remove, dims, grad, grad_dtype, ld_grad, None)

    bad_sides = [dict(qv=None), dict(qi=None), dict(pv=None), dict(pi=None), dict(mem_kind=7), dict(mem_kind=-1), dict(value_dtype=5),
                 dict(index_dtype=_lib.IDX_NONE), dict(index_dtype=9), dict(n_q=-1), dict(n_p=-4), dict(dims=0), dict(dims=-8), dict(ld_qv=7),
                 dict(ld_pi=4), dict(group=-1), dict(group=3), dict(group=1), dict(group=2, n_p=3)]
    for b in bad_sides:
        assert fwd(**b) == _lib.ERR_INVALID, b
        assert bwd(**b) == _lib.ERR_INVALID, b
    assert fwd(group=3) == _lib.ERR_INVALID and b"passage rows" in lib.dhr_last_error()
    for b in (dict(out=None), dict(ld_out=3), dict(ws_bytes=-1), dict(group=2, ld_out=1)):
        assert fwd(**b) == _lib.ERR_INVALID, b
    for b in (dict(g=None), dict(ld_g=3), dict(ld_dq=7), dict(ld_dp=0)):
        assert bwd(**b) == _lib.ERR_INVALID, b
    for b in (dict(dv=None), dict(idx=None), dict(grad=None), dict(mem_kind=3), dict(grad_dtype=2), dict(idx_dtype=_lib.IDX_NONE), dict(batch=-1),
              dict(vocab=0), dict(dims=0), dict(remove=-1), dict(remove=42), dict(ld_grad=41), dict(ld_dv=7), dict(ld_idx=7), dict(vocab=43), dict(dims=7)):
        assert dbw(**b) == _lib.ERR_INVALID, b
    assert dbw(remove=11) == _lib.ERR_INVALID and b"densified" in lib.dhr_last_error()
    # nothing to do: no device is touched
    assert fwd(n_q=0, n_p=0) == _lib.DHR_OK and bwd(dq=None, dp=None) == _lib.DHR_OK and dbw(batch=0) == _lib.DHR_OK
    assert lib.dhr_gip_scores_workspace(24, 192, 768, 0) > 0 and lib.dhr_gip_scores_workspace(24, 192, 768, 8) == 0
    assert lib.dhr_gip_scores_workspace(-1, 192, 768, 0) == 0 and lib.dhr_gip_scores_workspace(4096, 4096, 768, 0) == 0
    # valid calls: a status without a device, the result with one
    rcs = (fwd(), fwd(group=2, ld_out=2), bwd(), bwd(dq=None), bwd(group=2, ld_g=2), dbw(), dbw(grad_dtype=_lib.VAL_F16))
    want = _lib.DHR_OK if torch.cuda.is_available() else _lib.ERR_HIP
    assert all(rc == want for rc in rcs), rcs
    if not torch.cuda.is_available():
        from dhr_amd import gip_scores as GS
        with pytest.raises(_lib.DhrError, match="dhr_gip_scores failed"):
            GS.gip_scores(_A["qv"], _A["qi"], _A["pv"], _A["pi"])


def test_wrappers_raise_before_touching_the_library(monkeypatch):
    import torch
    from dhr_amd import gip_scores as GS

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    z = np.load(GOLDEN)
    texts = {e.split(" | ")[0]: e.split(" | ")[2] for e in z["errors"]}
    zeros = lambda rows, V=610: torch.zeros(rows, V)  # noqa: E731
    for make in (zeros, lambda rows, V=610: np.zeros((rows, V), np.float32)):
        with pytest.raises(ValueError) as e:
            GS.listwise_gip_scores(make(2, 611), make(6), 2, dims=8)
        assert str(e.value) == texts["listwise: vocabulary 611"]
        with pytest.raises(ValueError) as e:
            GS.listwise_gip_scores(make(2), make(6, 611), 2, dims=8)
        assert str(e.value) == texts["listwise: passages of vocabulary 611"]
        with pytest.raises(ValueError) as e:
            GS.pairwise_gip_scores(make(2)[:, None, :], make(6), 2, 3, dims=8)
        assert str(e.value) == texts["pairwise: 3-dimensional reps"]
        with pytest.raises(ValueError, match="cannot be densified"):
            GS.paired_gip_scores(make(2), make(2), dims=7)
        with pytest.raises(ValueError, match="cannot be densified"):
            GS.listwise_gip_scores(make(2), make(6), 2, dims=8, remove_dims=571)
        for bsz in (2, 4):                                        # query rows != effective_bsz
            with pytest.raises(RuntimeError, match=r"\(%d, 610\).*effective_bsz = %d" % (6 - bsz, bsz)):
                GS.listwise_gip_scores(make(6 - bsz), make(6), bsz, dims=8)
        for rows in (5, 12):                                      # passage rows != effective_bsz * train_n_passages
            with pytest.raises(RuntimeError, match=r"\(%d, 610\)" % rows):
                GS.pairwise_gip_scores(make(2), make(rows), 2, 3, dims=8)
        with pytest.raises(RuntimeError, match=r"\(3, 610\)"):
            GS.pairwise_gip_scores(make(3), make(6), 2, 3, dims=8)
        with pytest.raises(RuntimeError, match=r"\(3, 610\).*\(2, 610\)"):
            GS.paired_gip_scores(make(3), make(2), dims=8)
    with pytest.raises(RuntimeError, match="3 passage rows for 2 queries x 2"):
        GS.gip_scores(np.zeros((2, 8), np.float32), np.zeros((2, 8), np.uint8), np.zeros((3, 8), np.float32), np.zeros((3, 8), np.uint8), group=2)
    with pytest.raises(ValueError, match="one shape"):
        GS.gip_scores(np.zeros((2, 8), np.float32), np.zeros((2, 7), np.uint8), np.zeros((3, 8), np.float32), np.zeros((3, 8), np.uint8))


# ------------------------------------------------------------------------------------------ GPU part
def _call(GS, mode, tq, tp, dims, remove, bsz, n):
    if mode == "list":
        return GS.listwise_gip_scores(tq, tp, bsz, dims, remove)
    if mode == "pair":
        return GS.pairwise_gip_scores(tq, tp, bsz, n, dims, remove)
    return GS.paired_gip_scores(tq, tp, dims, remove)


def _check_fused(GS, key, q, p, dims, remove, bsz, n, mode, G, dtype="float32", req=(True, True), strided_g=False):
    """runs the fused call + backward on the device and checks scores and both [B, V] gradients against the restatement"""
    import torch
    tdt = getattr(torch, dtype)
    tq = torch.from_numpy(q).to("cuda", tdt).requires_grad_(req[0])
    tp = torch.from_numpy(p).to("cuda", tdt).requires_grad_(req[1])
    t = truth_reps(tq.detach().cpu().double().numpy(), tp.detach().cpu().double().numpy(), dims, remove, mode, G)
    s = _call(GS, mode, tq, tp, dims, remove, bsz, n)
    assert s.dtype == torch.float32 and tuple(s.shape) == ref_shape(mode, q.shape[0], p.shape[0]), (key, s.shape)
    assert_within(s.detach().cpu().numpy(), t["scores"], t["scores_bound"], key + " scores")
    tg = torch.from_numpy(np.asarray(G, np.float32)).cuda()
    if strided_g and tg.dim() == 2:
        tg = tg.t().contiguous().t()                             # the same numbers, columns contiguous
        assert not tg.is_contiguous() or 1 in tg.shape
    s.backward(tg)
    for side, x, needed in (("gq", tq, req[0]), ("gp", tp, req[1])):
        if not needed:
            assert x.grad is None
            continue
        assert x.grad.dtype == tdt and tuple(x.grad.shape) == tuple(x.shape)
        assert_within(x.grad.cpu().numpy(), t[side], t[side + "_bound"], f"{key} {side}", fp16=dtype == "float16")


@pytest.mark.gpu
def test_goldens_on_gpu():
    from dhr_amd import gip_scores as GS
    for key, z, q, p, dims, remove, bsz, n, mode in golden_cases():
        assert ref_shape(mode, q.shape[0], p.shape[0]) == z[key + "_scores"].shape
        _check_fused(GS, key, q, p, dims, remove, bsz, n, mode, z[key + "_G"])
        _check_fused(GS, key + " fp16", q, p, dims, remove, bsz, n, mode, z[key + "_G"], dtype="float16")


def _random_reps(rng, rows, dims, groups, remove, density, negative, exact=True):
    """exact: multiples of 2^-6 (fp16 holds them; with G in multiples of 2^-4 no gradient leaves fp16's normal range); else any fp32 value"""
    V = remove + groups * dims
    x = rng.uniform(0.05, 3.0, (rows, V))
    if exact:
        x = np.round(x * 64) / 64
    if negative:
        x = x * rng.choice([-1.0, 1.0], (rows, V))
    return (x * (rng.random((rows, V)) < density)).astype(np.float32)


def _random_g(rng, shape, exact=True):
    g = rng.uniform(-2.0, 2.0, shape)
    if exact:
        g = np.round(g * 16) / 16
        g[g == 0] = 0.0625
    return g.astype(np.float32)


# (n_q, passages per query (pair) or passage rows (list / one), mode, dims, groups, remove, density, dtype, requires_grad, strided G)
RANDOM_CASES = [
    (1, 7, "list", 96, 5, 10, 0.5, "float32", (True, True), False),
    (200, 37, "list", 40, 3, 0, 0.7, "float16", (True, True), True),
    (33, 3, "pair", 100, 7, 570, 0.3, "float32", (True, False), False),
    (17, 129, "list", 768, 39, 570, 0.02, "float16", (False, True), True),
    (65, 2, "pair", 70, 300, 3, 0.02, "float32", (True, True), True),
    (100, 200, "list", 520, 2, 570, 0.6, "float32", (True, True), False),       # 32 x 64 tiles, dims split with a short last slice
    (9, 4, "pair", 33, 4, 1, 1.0, "float16", (False, True), False),
    (13, 13, "one", 50, 6, 570, 0.4, "float16", (True, True), False),
    (1, 19, "one", 50, 6, 570, 0.4, "float32", (True, True), False),
    (21, 1, "one", 768, 39, 570, 0.05, "float32", (True, False), False),
    (47, 1, "pair", 64, 9, 0, 0.5, "float32", (True, True), False),
]


@pytest.mark.gpu
def test_random_cases_against_restatement():
    """No exemptions: every entry of the scores and of both gradients inside the bound."""
    from dhr_amd import gip_scores as GS
    rng = np.random.default_rng(7)
    for k, (n_q, m, mode, dims, groups, remove, density, dtype, req, strided) in enumerate(RANDOM_CASES):
        n_p = n_q * m if mode == "pair" else m
        exact = dtype == "float16"                             # fp32 cases draw unrounded values: their sums do round
        q = _random_reps(rng, n_q, dims, groups, remove, density, k % 2 == 1, exact)
        p = _random_reps(rng, n_p, dims, groups, remove, density, k % 2 == 1, exact)
        G = _random_g(rng, ref_shape(mode, n_q, n_p), exact)
        _check_fused(GS, f"random[{k}] {mode} {n_q}x{n_p} dims {dims} {dtype}", q, p, dims, remove, n_q, m if mode == "pair" else 1, mode, G,
                     dtype=dtype, req=req, strided_g=strided)


@pytest.mark.gpu
def test_gip_scores_on_strided_record_views():
    """gip_scores on the [:, :dims] views of [value | cls] records, every index dtype, listwise and pairwise; numpy in -> numpy out; and the
    unsplit forward (no workspace) of a shape the wrapper runs split."""
    import torch
    from dhr_amd import gip_scores as GS
    rng = np.random.default_rng(11)
    for k, (n_q, n, group, dims, groups, vdt, idt) in enumerate([(5, 11, 0, 24, 5, "float16", "uint8"), (37, 3, 3, 100, 100, "float32", "int8"),
                                                                 (100, 200, 0, 520, 300, "float32", "int16"), (3, 70, 0, 64, 9, "float16", "int64")]):
        n_p = n_q * n if group else n
        rec = {}
        for side, rows in (("q", n_q), ("p", n_p)):
            v = np.zeros((rows, dims + 16), np.float32)
            v[:, :dims] = rng.uniform(-3, 3, (rows, dims)) if vdt == "float32" else np.round(rng.uniform(-3, 3, (rows, dims)) * 64) / 64
            v[:, dims:] = 7.0                                                             # the CLS tail must not be read
            i = np.full((rows, dims + 3), 1, np.int64)
            i[:, :dims] = rng.integers(0, groups, (rows, dims)) - (64 if idt == "int8" else 0)
            rec[side] = (torch.from_numpy(v).to("cuda", getattr(torch, vdt)).requires_grad_(True), torch.from_numpy(i).to("cuda", getattr(torch, idt)))
        (rqv, rqi), (rpv, rpi) = rec["q"], rec["p"]
        pairs = pairs_of("pair" if group else "list", n_q, n_p)
        G = np.zeros((n_q, n_p))
        Gs = _random_g(rng, (n_q, group if group else n_p), vdt == "float16")
        G[pairs] = Gs.reshape(-1)
        f64 = lambda t: t.detach().cpu().double().numpy()  # noqa: E731
        S, bS, dq, bq, dp, bp = truth_scores(f64(rqv)[:, :dims], f64(rqi)[:, :dims], f64(rpv)[:, :dims], f64(rpi)[:, :dims], G, pairs)
        s = GS.gip_scores(rqv[:, :dims], rqi[:, :dims], rpv[:, :dims], rpi[:, :dims], group)
        assert s.dtype == torch.float32 and tuple(s.shape) == Gs.shape
        assert_within(s.detach().cpu().numpy(), S[pairs].reshape(Gs.shape), bS[pairs].reshape(Gs.shape), f"records[{k}] scores")
        s.backward(torch.from_numpy(Gs).cuda())
        for name, rv, d, b in (("dq", rqv, dq, bq), ("dp", rpv, dp, bp)):
            assert rv.grad.dtype == rv.dtype
            g = rv.grad.cpu().numpy()
            assert not g[:, dims:].any()
            assert_within(g[:, :dims], d, b, f"records[{k}] {name}", fp16=vdt == "float16")
        # numpy in -> numpy out (staged through the device), the same bits
        s_np = GS.gip_scores(rqv.detach().cpu().numpy()[:, :dims], rqi.cpu().numpy()[:, :dims], rpv.detach().cpu().numpy()[:, :dims],
                             rpi.cpu().numpy()[:, :dims], group)
        assert isinstance(s_np, np.ndarray) and np.array_equal(s_np, s.detach().cpu().numpy())
        if k == 2:                                              # the same problem without a workspace: unsplit, another order, the same bound
            lib = _lib.load()
            qv, pv = rqv.detach()[:, :dims], rpv.detach()[:, :dims]
            qi, pi = rqi[:, :dims], rpi[:, :dims]
            assert lib.dhr_gip_scores_workspace(n_q, n_p, dims, 0) > 0
            out = torch.full((n_q, n_p + 5), -1.0, device="cuda")
            _lib.check(lib.dhr_gip_scores(0, _lib.MEM_DEVICE, qv.data_ptr(), qv.stride(0), qi.data_ptr(), qi.stride(0), n_q, pv.data_ptr(), pv.stride(0),
                                          pi.data_ptr(), pi.stride(0), n_p, dims, _lib.VAL_F32, _lib.IDX_I16, 0, out.data_ptr(), out.stride(0), None, 0,
                                          None), "dhr_gip_scores")
            torch.cuda.synchronize()
            assert_within(out[:, :n_p].cpu().numpy(), S, bS, "records[2] scores, unsplit")
            assert (out[:, n_p:] == -1.0).all()


# (n_q, passages per query (group > 0) or passage rows, group, dims): what the launchers of gip_train.hip decide by the shape alone
ARM_SHAPES = {"list, 16 x 16 tiles, one gradient row per thread": (5, 11, 0, 24),
              "pairwise": (7, 3, 3, 40),
              "list, 32 x 64 tiles, two (dq) and four (dp) gradient rows per thread": (512, 1024, 0, 64)}
_ARM_CASES = {}


def _arm_case(name):
    """-> (qv, qi, pv, pi, Gs, truth of truth_scores), made once and left unchanged: values in multiples of 2^-6 and G in multiples of 2^-4
    (exact in fp16), groups in [0, 100), or in [0, 4) at 64 dims so that the long gradient sums have many terms (every index dtype holds them)"""
    if name not in _ARM_CASES:
        n_q, n, group, dims = ARM_SHAPES[name]
        n_p = n_q * n if group else n
        rng = np.random.default_rng([19, n_q, n_p, dims])
        qv, pv = (np.round(rng.uniform(-3, 3, (rows, dims)) * 64) / 64 for rows in (n_q, n_p))
        qi, pi = (rng.integers(0, 100 if dims < 64 else 4, (rows, dims)) for rows in (n_q, n_p))
        pairs = pairs_of("pair" if group else "list", n_q, n_p)
        Gs = _random_g(rng, (n_q, group if group else n_p), True)
        G = np.zeros((n_q, n_p))
        G[pairs] = Gs.reshape(-1)
        t = truth_scores(qv, qi, pv, pi, G, pairs)
        _ARM_CASES[name] = (qv, qi, pv, pi, Gs, pairs, tuple(x[pairs].reshape(Gs.shape) for x in t[:2]) + t[2:])
    return _ARM_CASES[name]


@pytest.mark.gpu
@pytest.mark.parametrize("idt", ["uint8", "int8", "int16"])
@pytest.mark.parametrize("vdt", ["float32", "float16"])
@pytest.mark.parametrize("name", list(ARM_SHAPES))
def test_every_value_and_index_type_at_every_launch_shape(name, vdt, idt):
    """Both value types with each of the three index types through gip_scores and its backward, at a shape for every arm the launchers pick:
    the small and the large forward tile, the pairwise kernels, and one, two and four gradient rows per thread (512 and 1024 rows of 64 dims
    on the differentiated side).  Scores and both gradients inside the bounds of the restatement."""
    import torch
    from dhr_amd import gip_scores as GS
    n_q, n, group, dims = ARM_SHAPES[name]
    qv, qi, pv, pi, Gs, pairs, (S, bS, dq, bq, dp, bp) = _arm_case(name)
    tv, ti = getattr(torch, vdt), getattr(torch, idt)
    tqv, tpv = (torch.from_numpy(x).to("cuda", tv).requires_grad_(True) for x in (qv, pv))
    tqi, tpi = (torch.from_numpy(x).to("cuda", ti) for x in (qi, pi))
    s = GS.gip_scores(tqv, tqi, tpv, tpi, group)
    what = f"{name} {vdt} {idt}"
    assert s.dtype == torch.float32 and tuple(s.shape) == Gs.shape
    assert_within(s.detach().cpu().numpy(), S, bS, what + " scores")
    s.backward(torch.from_numpy(Gs).cuda())
    for side, x, d, b in (("dq", tqv, dq, bq), ("dp", tpv, dp, bp)):
        assert x.grad.dtype == tv and x.grad.any()
        assert_within(x.grad.cpu().numpy(), d, b, f"{what} {side}", fp16=vdt == "float16")


@pytest.mark.gpu
@pytest.mark.parametrize("idt", ["uint8", "int8", "int16"])
@pytest.mark.parametrize("odt", ["float32", "float16"])
def test_densify_backward_of_every_index_and_output_type(idt, odt):
    """dL/dvalue [5, 24] in multiples of 2^-6 and groups below 7 of each index dtype -> dL/dreps [5, 10 + 7 * 24] in fp32 and in fp16:
    the scatter of the restatement, exactly (densify itself produces uint8 or int16 groups only)."""
    import torch
    from dhr_amd import gip_scores as GS
    rng = np.random.default_rng(23)
    B, dims, groups, remove = 5, 24, 7, 10
    vocab = remove + groups * dims
    dv = np.round(rng.uniform(-3, 3, (B, dims)) * 64) / 64
    idx = rng.integers(0, groups, (B, dims))
    got = GS._densify_bwd(torch.from_numpy(dv).float().cuda(), torch.from_numpy(idx).to("cuda", getattr(torch, idt)), vocab, dims, remove,
                          getattr(torch, odt))
    assert got.dtype == getattr(torch, odt) and tuple(got.shape) == (B, vocab)
    assert np.array_equal(got.cpu().numpy().astype(np.float64), scatter(dv, idx, vocab, dims, remove)) and got.any()


@pytest.mark.gpu
def test_fused_equals_composed_and_runs_are_bit_identical():
    import torch
    from dhr_amd import gip_scores as GS
    from dhr_amd.densify import densify
    rng = np.random.default_rng(13)
    for n_q, m, mode, dims, groups, remove, dtype in ((24, 192, "list", 768, 39, 570, "float32"), (100, 200, "list", 520, 2, 570, "float16"),
                                                      (31, 5, "pair", 768, 39, 570, "float16"), (7, 50, "list", 8, 300, 570, "float32")):
        n_p = n_q * m if mode == "pair" else m
        group = m if mode == "pair" else 0
        q = torch.from_numpy(_random_reps(rng, n_q, dims, groups, remove, 0.05, True)).to("cuda", getattr(torch, dtype))
        p = torch.from_numpy(_random_reps(rng, n_p, dims, groups, remove, 0.05, True)).to("cuda", getattr(torch, dtype))
        G = torch.from_numpy(_random_g(rng, (n_q, m))).cuda()
        runs = []
        for _ in range(2):
            tq, tp = q.clone().requires_grad_(True), p.clone().requires_grad_(True)
            s = _call(GS, mode, tq, tp, dims, remove, n_q, m)
            s.backward(G)
            runs.append((s.detach(), tq.grad, tp.grad))
        for a, b in zip(*runs):
            assert torch.equal(a, b)
        qv, qi = densify(q, dims, remove_dims=remove)
        pv, pi = densify(p, dims, remove_dims=remove)
        assert qi.dtype == torch.int64
        qv.requires_grad_(True)
        pv.requires_grad_(True)
        s2 = GS.gip_scores(qv, qi, pv, pi, group)
        s2.backward(G)
        assert torch.equal(s2.detach(), runs[0][0])
        cols_q = remove + qi * dims + torch.arange(dims, device="cuda")[None, :]
        cols_p = remove + pi * dims + torch.arange(dims, device="cuda")[None, :]
        assert torch.equal(runs[0][1].gather(1, cols_q), qv.grad) and torch.equal(runs[0][2].gather(1, cols_p), pv.grad)
        assert int((runs[0][1] != 0).sum()) == int((qv.grad != 0).sum()) and int((runs[0][2] != 0).sum()) == int((pv.grad != 0).sum())


@pytest.mark.gpu
def test_memory_stays_far_below_one_byte_per_pair_and_slice():
    """(n_q, n_p) = (96, 768), V = 30522, fp32: the peak over forward + backward, minus what was allocated before the call and minus the tensors
    the call returns (scores and the two .grad), stays below n_q * n_p * dims BYTES: less than any materialised [n_q, n_p, dims] temporary."""
    import torch
    from dhr_amd import gip_scores as GS
    n_q, n_p, V, dims = 96, 768, 30522, 768
    gen = torch.Generator(device="cuda").manual_seed(3)
    q = torch.rand((n_q, V), device="cuda", generator=gen).requires_grad_(True)
    p = torch.rand((n_p, V), device="cuda", generator=gen).requires_grad_(True)
    G = torch.rand((n_q, n_p), device="cuda", generator=gen)
    GS.listwise_gip_scores(q, p, n_q).backward(G)                 # warm-up: the library is loaded, kernels are resident
    q.grad = p.grad = None
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    s = GS.listwise_gip_scores(q, p, n_q)
    s.backward(G)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    returned = sum(t.numel() * t.element_size() for t in (s, q.grad, p.grad))
    extra = peak - before - returned
    print(f"memory: peak {peak - before} B over the call, returned tensors {returned} B, the op's own {extra} B; limit {n_q * n_p * dims} B")
    assert extra < n_q * n_p * dims


def _eager(q_reps, p_reps, bsz, dims=768, remove=570):
    """The eager torch composition of the listwise score (densify both sides, the passage batch repeated once per query, the equality mask,
    a batched matmul), restated: the baseline of the timing printout."""
    B, P = q_reps.shape[0], p_reps.shape[0]
    qv, qi = q_reps[:, remove:].view(B, -1, dims).max(1)
    pv, pi = p_reps[:, remove:].view(P, -1, dims).max(1)
    qv, qi = qv.view(bsz, 1, -1), qi.view(bsz, 1, -1)
    pv, pi = pv[None].repeat((bsz, 1, 1)), pi[None].repeat((bsz, 1, 1))
    pv = (pi == qi) * pv
    return (qv @ pv.transpose(2, 1)).squeeze()


@pytest.mark.gpu
def test_timing_printout():
    """Forward + backward of the listwise score from [B, 30522] fp32 reps, this library against the eager torch composition, alternating:
    device events around windows of 50 iterations after a warm-up, three repeats so the spread shows.  A printout, never a threshold."""
    import torch
    from dhr_amd import gip_scores as GS
    V, iters = 30522, 50
    for n_q, n_p in ((24, 192), (96, 768), (192, 1536)):
        gen = torch.Generator(device="cuda").manual_seed(n_q)
        q = (torch.rand((n_q, V), device="cuda", generator=gen) * (torch.rand((n_q, V), device="cuda", generator=gen) < 0.02)).requires_grad_(True)
        p = (torch.rand((n_p, V), device="cuda", generator=gen) * (torch.rand((n_p, V), device="cuda", generator=gen) < 0.05)).requires_grad_(True)
        G = torch.randn((n_q, n_p), device="cuda", generator=gen)

        def step(fn):
            q.grad = p.grad = None
            fn(q, p, n_q).backward(G)

        def window(fn, n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                step(fn)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / n

        times = {"fused": [], "eager": []}
        for _ in range(3):
            for name, fn in (("fused", GS.listwise_gip_scores), ("eager", _eager)):
                window(fn, 5)
                times[name].append(window(fn, iters))
                q.grad = p.grad = None
                torch.cuda.empty_cache()                          # the eager side keeps several GB at the largest shape
        f, e = times["fused"], times["eager"]
        print(f"gip scores fwd+bwd n_q={n_q} n_p={n_p} V={V} fp32: fused " + " / ".join(f"{t:.3f}" for t in f) + " ms, eager torch " +
              " / ".join(f"{t:.3f}" for t in e) + f" ms, {np.median(e) / np.median(f):.1f}x")
        del q, p, G
        torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("group,n_p", [(0, 4), (2, 6)])
def test_host_arrays_with_row_strides_match_the_device_path(group, n_p):
    """n_q = 3, dims = 8, every operand of the three entry points a host array cut from a wider base (row stride > row): staged through the
    device, complete on return, and the bits of the same views processed on the device.  The columns beside an output stay untouched."""
    import torch
    from dhr_amd import gip_scores as GS
    lib = _lib.load()
    n_q, dims, W = 3, 8, 12
    cols = group or n_p
    rng = np.random.default_rng(5)
    bqv, bpv = (rng.uniform(-2, 2, (n, W)).astype(np.float32) for n in (n_q, n_p))
    bqi, bpi = (rng.integers(0, 4, (n, W)).astype(np.uint8) for n in (n_q, n_p))
    bG = rng.uniform(-1, 1, (n_q, cols + 3)).astype(np.float32)
    out, dq, dp = (np.full((n, c + 2), 7, np.float32) for n, c in ((n_q, cols), (n_q, dims), (n_p, dims)))
    sides = (bqv.ctypes.data, W, bqi.ctypes.data, W, n_q, bpv.ctypes.data, W, bpi.ctypes.data, W, n_p, dims, _lib.VAL_F32, _lib.IDX_U8, group)
    assert lib.dhr_gip_scores(0, _lib.MEM_HOST, *sides, out.ctypes.data, cols + 2, None, 0, None) == _lib.DHR_OK, lib.dhr_last_error()
    assert lib.dhr_gip_scores_backward(0, _lib.MEM_HOST, *sides, bG.ctypes.data, cols + 3, dq.ctypes.data, dims + 2, dp.ctypes.data, dims + 2,
                                       None) == _lib.DHR_OK, lib.dhr_last_error()
    dev = lambda a, n: torch.from_numpy(a).cuda()[:, :n]   # noqa: E731
    tq, tp = dev(bqv, dims).requires_grad_(True), dev(bpv, dims).requires_grad_(True)
    s = GS.gip_scores(tq, dev(bqi, dims), tp, dev(bpi, dims), group)
    s.backward(dev(bG, cols))
    for host, n, t in ((out, cols, s.detach()), (dq, dims, tq.grad), (dp, dims, tp.grad)):
        assert np.array_equal(host[:, :n], t.cpu().numpy()) and (host[:, n:] == 7).all()
    # dhr_densify_backward: dL/dvalue [n_q, 8] and the groups of the query side -> dL/dreps [n_q, 42] (10 removed columns, 4 groups of 8)
    vocab, remove = 42, 10
    bdv = rng.uniform(-1, 1, (n_q, W)).astype(np.float32)
    grad = np.full((n_q, vocab + 2), 7, np.float32)
    assert lib.dhr_densify_backward(0, _lib.MEM_HOST, bdv.ctypes.data, W, bqi.ctypes.data, _lib.IDX_U8, W, n_q, vocab, remove, dims, grad.ctypes.data,
                                    _lib.VAL_F32, vocab + 2, None) == _lib.DHR_OK, lib.dhr_last_error()
    want = GS._densify_bwd(dev(bdv, dims), dev(bqi, dims), vocab, dims, remove, torch.float32)
    assert np.array_equal(grad[:, :vocab], want.cpu().numpy()) and (grad[:, vocab:] == 7).all()
