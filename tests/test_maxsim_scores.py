"""Differentiable late-interaction (MaxSim) scores (dhr_amd/maxsim_scores.py on dhr_maxsim_scores / dhr_maxsim_scores_backward).

Truth is the float64 restatement below: an einsum for the similarities, a first-wins argmax over passage tokens, gradients written out by
hand (no autograd).  The golden fixture (the reference's own methods, tests/golden/make_golden_maxsim.py) holds values on a grid on which
every product and sum is exact in fp32, so the library must reproduce it bit for bit, ties included (an fp16 gradient is the exact value
rounded once).  For continuous inputs the tolerance is derived, not measured: a similarity may be off by (D + 2) * 2^-24 * sum_k |q_k p_k|,
a score by the sum of that over i at the winning tokens, a gradient entry by (n + 2) * 2^-24 * sum|terms| with n the number of summed terms,
plus 2^-11 * |truth| where the output is fp16.  There is no absolute term: where every term is zero the result must be exactly zero.
Gradients are comparable only where the winner is unambiguous: the seeded cases assert, from the float64 similarities alone, that every
(a, b, i) keeps its best and second-best similarity further apart than twice the similarity bound.

CPU part (-m "not gpu"): the fixture against the restatement, statuses of the two entry points, the wrappers' errors.  GPU part: goldens,
seeded random cases, a recipe-sized step, views, bit-identity, memory, a timing printout."""
import os

import numpy as np
import pytest

from dhr_amd import _lib, _marshal

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "maxsim_golden.npz")
U32, U16 = 2.0 ** -24, 2.0 ** -11
MODES = ("list", "pair", "one")


# ------------------------------------------------------------------------------------------ float64 restatement
def pairs_of(mode, A, B, n):
    """list: all pairs; pair: passage row a * n + j belongs to query a; one: row a with row a"""
    if mode == "list":
        return np.ones((A, B), bool)
    n = n if mode == "pair" else 1
    return (np.arange(B)[None, :] // n) == np.arange(A)[:, None]


def ref_shape(mode, A, B, n):
    """what the reference returns: listwise unsqueezed, pairwise squeezed, paired [A]"""
    if mode == "list":
        return (A, B)
    if mode == "one":
        return (A,)
    return tuple(d for d in (A, n) if d != 1)


def truth(q, p, G, pairs):
    """q [A, Lq, D], p [B, Lp, D] float64; G [A, B] (zero outside `pairs`); pairs bool [A, B]: the scored pairs.
    -> dict: S, bS [A, B]; arg [A, B, Lq]; gap, bsim [A, B, Lq] (best minus second-best similarity, the largest similarity bound of the
    row); dq, bq [A, Lq, D]; dp, bp [B, Lp, D]."""
    A, Lq, D = q.shape
    B, Lp, _ = p.shape
    sim = np.einsum("aik,bjk->abij", q, p)
    bsim = (D + 2) * U32 * np.einsum("aik,bjk->abij", np.abs(q), np.abs(p))
    arg = sim.argmax(-1)                                          # numpy's argmax returns the first maximum
    best = np.take_along_axis(sim, arg[..., None], -1)[..., 0]
    S = (best * pairs[:, :, None]).sum(-1)
    bS = (np.take_along_axis(bsim, arg[..., None], -1)[..., 0] * pairs[:, :, None]).sum(-1)
    if Lp > 1:
        second = np.partition(sim, Lp - 2, axis=-1)[..., Lp - 2]
        gap = best - second
    else:
        gap = np.full(best.shape, np.inf)
    won = (arg[..., None] == np.arange(Lp)) * pairs[:, :, None, None]          # [A, B, Lq, Lp]
    Gp = G * pairs
    pw = np.take_along_axis(p[None], arg[..., None], 2)           # p[b][arg[a][b][i]]: [A, B, Lq, D]
    dq = np.einsum("ab,abid->aid", Gp, pw)
    bq = (int(pairs.sum(1).max()) + 2) * U32 * np.einsum("ab,abid->aid", np.abs(Gp), np.abs(pw))
    dp = np.einsum("ab,abij,aid->bjd", Gp, won, q)
    n_terms = won.sum((0, 2))                                     # [B, Lp]
    bp = (n_terms[:, :, None] + 2) * U32 * np.einsum("ab,abij,aid->bjd", np.abs(Gp), won, np.abs(q))
    return dict(S=S, bS=bS, arg=arg, gap=gap, bsim=bsim.max(-1), dq=dq, bq=bq, dp=dp, bp=bp)


def full_g(G_ref, pairs):
    G = np.zeros(pairs.shape)
    G[pairs] = np.asarray(G_ref, np.float64).reshape(-1)
    return G


def assert_within(got, want, bound, what, fp16=False):
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    tol = bound + (U16 * np.abs(want) if fp16 else 0.0)
    err = np.abs(got - want)
    bad = err > tol
    worst = float((err / np.where(tol > 0, tol, 1.0))[tol > 0].max()) if (tol > 0).any() else 0.0
    print(f"{what}: max error / bound = {worst:.4f}, entries with a zero bound that are not zero: {int((err[tol == 0] != 0).sum())}")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} entries outside the bound (worst error / bound {worst:.3f})"


def golden_cases():
    z = np.load(GOLDEN)
    for name in z["names"]:
        A, B, n, Lq, Lp, D = (int(v) for v in z[name + "_geom"])
        for mode in MODES:
            p8 = z[name + "_p"] if mode != "one" else np.ascontiguousarray(z[name + "_p"][::n])
            yield f"{name}_{mode}", z, z[name + "_q"].astype(np.float64) / 8, p8.astype(np.float64) / 8, n, mode


# ------------------------------------------------------------------------------------------ CPU part
def test_fixture_matches_float64_restatement():
    seen = 0
    for key, z, q, p, n, mode in golden_cases():
        A, B = q.shape[0], p.shape[0]
        pairs = pairs_of(mode, A, B, n)
        t = truth(q, p, full_g(z[key + "_G"], pairs), pairs)
        shape = ref_shape(mode, A, B, n)
        assert z[key + "_scores"].shape == shape and z[key + "_G"].shape == shape, key
        assert z[key + "_scores"].dtype == np.float32 and q.shape[2] <= 768
        assert np.array_equal(z[key + "_scores"].astype(np.float64), t["S"][pairs].reshape(shape)), key
        assert np.array_equal(z[key + "_gq"] / 128.0, t["dq"]), key
        assert np.array_equal(z[key + "_gp"] / 128.0, t["dp"]), key
        seen += 1
    assert seen == 24
    # the designed cases do what they were designed for
    q, p = z["base_q"].astype(np.float64) / 8, z["base_p"].astype(np.float64) / 8
    assert q.shape == (4, 31, 128) and p.shape == (12, 149, 128) and not p[:, 140:].any() and not q[1, 26:].any()
    pairs = pairs_of("list", 4, 12, 3)
    t = truth(q, p, full_g(z["base_list_G"], pairs), pairs)
    assert np.array_equal(p[1, 2], p[1, 5]) and t["arg"][0, 1, 3] == 2 and t["gap"][0, 1, 3] == 0                # two equal tokens: the first
    assert t["arg"][2, 6, 7] == 140 and (np.einsum("k,jk->j", q[2, 7], p[6, :140]) < 0).all()                    # all negative: the first padded token, at 0
    assert not t["arg"][1, :, 26:].any()                                                                        # all-zero query tokens: token 0
    assert int((t["gap"] == 0).sum()) - 5 * 12 >= 3                                                             # exact ties beyond the zero tokens
    assert z["base_list_gp"][6, 140].any() and not z["base_list_gp"][1, 5].any()
    q, p = z["edge_q"].astype(np.float64) / 8, z["edge_p"].astype(np.float64) / 8
    assert q.shape == (2, 33, 32) and p.shape == (4, 65, 32)
    pairs = pairs_of("list", 2, 4, 2)
    t = truth(q, p, full_g(z["edge_list_G"], pairs), pairs)
    assert t["arg"][0, 0, 32] == 64 and t["arg"][0, 0, 0] == 64 and t["arg"][0, 1, 5] == 0 and t["arg"][1, 1, 32] == 0 and t["arg"][0, 2, 32] == 0
    assert z["cls_q"].shape == (4, 1, 128) and z["d20_p"].shape == (6, 7, 20) and z["lp32_p"].shape == (4, 32, 32) and z["d768_p"].shape == (4, 40, 768)
    assert z["a1_pair_scores"].shape == (3,) and z["n1_pair_scores"].shape == (4,) and z["a1_list_scores"].shape == (1, 3)
    assert [e.split(" | ")[1] for e in z["errors"]] == ["RuntimeError", "RuntimeError"]


_A = dict(q=np.ones((2, 3, 8), np.float32), p=np.ones((4, 5, 8), np.float32), out=np.zeros((2, 4), np.float32), arg=np.zeros((2, 4, 3), np.int16),
          g=np.ones((2, 4), np.float32), dq=np.zeros((2, 3, 8), np.float32), dp=np.zeros((4, 5, 8), np.float32))


def _args(**kw):
    """valid host arguments of dhr_maxsim_scores / _backward (2 queries x 3 tokens, 4 passages x 5 tokens, 8 dims), with overrides"""
    a = dict(device=0, mem_kind=_lib.MEM_HOST, q=_A["q"].ctypes.data, ld_q_tok=8, ld_q_batch=24, A=2, Lq=3, p=_A["p"].ctypes.data, ld_p_tok=8, ld_p_batch=40,
             B=4, Lp=5, D=8, value_dtype=_lib.VAL_F32, group=0)
    a.update(kw)
    return list(a.values())


def test_entry_points_return_statuses():
    import torch
    lib = _lib.load()
    for name in ("dhr_maxsim_scores", "dhr_maxsim_scores_backward"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert lib.dhr_version() == 105
    out, arg, g, dq, dp = (_A[k].ctypes.data for k in ("out", "arg", "g", "dq", "dp"))

    def fwd(out=out, ld_out=4, arg=arg, **kw):
        return lib.dhr_maxsim_scores(*_args(**kw), out, ld_out, arg, None)

    def bwd(arg=arg, g=g, ld_g=4, dq=dq, dp=dp, grad_dtype=_lib.VAL_F32, **kw):
        return lib.dhr_maxsim_scores_backward(*_args(**kw), arg, g, ld_g, dq, dp, grad_dtype, None)

    invalid = [dict(q=None), dict(p=None), dict(mem_kind=7), dict(mem_kind=-1), dict(value_dtype=5), dict(value_dtype=-1), dict(A=-1), dict(B=-4),
               dict(Lq=0), dict(Lq=-3), dict(Lp=0), dict(D=0), dict(D=-8), dict(ld_q_tok=7), dict(ld_p_tok=0), dict(ld_q_batch=7), dict(ld_p_batch=-40),
               dict(group=-1), dict(group=3), dict(group=1), dict(group=2, B=3)]
    for b in invalid:
        assert fwd(**b) == _lib.ERR_INVALID and lib.dhr_last_error(), b
        assert bwd(**b) == _lib.ERR_INVALID and lib.dhr_last_error(), b
    assert fwd(group=3) == _lib.ERR_INVALID and b"passage rows" in lib.dhr_last_error()
    unsupported = [dict(D=1025, ld_q_tok=1025, ld_p_tok=1025, ld_q_batch=4096, ld_p_batch=8192), dict(Lp=32768), dict(A=1 << 18), dict(B=1 << 18)]
    for b in unsupported:
        assert fwd(**b) == _lib.ERR_UNSUPPORTED and lib.dhr_last_error(), b
        assert bwd(**b) == _lib.ERR_UNSUPPORTED and lib.dhr_last_error(), b
    assert fwd(Lp=32768) == _lib.ERR_UNSUPPORTED and b"32767" in lib.dhr_last_error()
    for b in (dict(out=None), dict(ld_out=3), dict(group=2, ld_out=1)):
        assert fwd(**b) == _lib.ERR_INVALID, b
    for b in (dict(arg=None), dict(g=None), dict(ld_g=3), dict(grad_dtype=2), dict(grad_dtype=-1), dict(group=2, ld_g=1)):
        assert bwd(**b) == _lib.ERR_INVALID, b
    # nothing to do: no device is touched
    assert fwd(A=0, B=0) == _lib.DHR_OK and fwd(B=0) == _lib.DHR_OK and bwd(dq=None, dp=None) == _lib.DHR_OK and bwd(A=0, B=0) == _lib.DHR_OK
    # valid calls: a status without a device, the result with one
    rcs = (fwd(), fwd(arg=None), fwd(group=2, ld_out=2), bwd(), bwd(dq=None), bwd(dp=None, grad_dtype=_lib.VAL_F16), bwd(group=2, ld_g=2))
    want = _lib.DHR_OK if torch.cuda.is_available() else _lib.ERR_HIP
    assert all(rc == want for rc in rcs), rcs
    if not torch.cuda.is_available():
        from dhr_amd import maxsim_scores as MS
        with pytest.raises(_lib.DhrError, match="dhr_maxsim_scores failed"):
            MS.maxsim_scores(_A["q"], _A["p"])


def test_wrappers_raise_before_touching_the_library(monkeypatch):
    import torch
    from dhr_amd import maxsim_scores as MS

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    for make in (lambda *s: torch.zeros(*s), lambda *s: np.zeros(s, np.float32), lambda *s: torch.zeros(*s, requires_grad=True)):
        with pytest.raises(RuntimeError, match="16 dims, passages 20"):         # the reference: RuntimeError from einsum
            MS.listwise_maxsim(make(2, 5, 16), make(6, 7, 20))
        for rows in (5, 12):                                                    # the reference: RuntimeError from view (5 rows)
            with pytest.raises(RuntimeError, match=r"\(%d, 7, 16\).*2 queries x train_n_passages = 3" % rows):
                MS.pairwise_maxsim(make(2, 5, 16), make(rows, 7, 16), 3)
        with pytest.raises(RuntimeError, match="train_n_passages = 0"):
            MS.pairwise_maxsim(make(2, 5, 16), make(6, 7, 16), 0)
        with pytest.raises(RuntimeError, match="do not pair up"):
            MS.paired_maxsim(make(3, 5, 16), make(2, 7, 16))
        with pytest.raises(RuntimeError, match="5 passage rows for 2 queries x 2"):
            MS.maxsim_scores(make(2, 5, 16), make(5, 7, 16), group=2)
        with pytest.raises(RuntimeError, match="group|passage rows"):
            MS.maxsim_scores(make(2, 5, 16), make(4, 7, 16), group=-1)
        with pytest.raises(ValueError, match=r"\[batch, tokens, dims\]"):
            MS.listwise_maxsim(make(2, 16), make(6, 7, 16))
        with pytest.raises(ValueError, match=r"\[batch, tokens, dims\]"):
            MS.maxsim_scores(make(2, 5, 16), make(6, 7, 2, 8))
        with pytest.raises(ValueError, match="empty"):
            MS.maxsim_scores(make(2, 0, 16), make(6, 7, 16))
        with pytest.raises(_lib.DhrError, match="1024 dims") as e:
            MS.maxsim_scores(make(1, 2, 1025), make(1, 2, 1025))
        assert e.value.status == _lib.ERR_UNSUPPORTED
        with pytest.raises(_lib.DhrError, match="32767 passage tokens"):
            MS.maxsim_scores(make(1, 2, 4), make(1, 32768, 4))
    with pytest.raises(TypeError, match="cannot be mixed"):
        MS.maxsim_scores(np.zeros((2, 5, 16), np.float32), torch.zeros(6, 7, 16))


# ------------------------------------------------------------------------------------------ GPU part
def _call(MS, mode, tq, tp, n):
    if mode == "list":
        return MS.listwise_maxsim(tq, tp)
    if mode == "pair":
        return MS.pairwise_maxsim(tq, tp, n)
    return MS.paired_maxsim(tq, tp)


def _run(MS, mode, q, p, n, G, dtype, req=(True, True)):
    """-> (scores, dq or None, dp or None) as numpy arrays, from device tensors of `dtype`"""
    import torch
    tdt = getattr(torch, dtype)
    tq = torch.from_numpy(np.asarray(q, np.float32)).to("cuda", tdt).requires_grad_(req[0])
    tp = torch.from_numpy(np.asarray(p, np.float32)).to("cuda", tdt).requires_grad_(req[1])
    s = _call(MS, mode, tq, tp, n)
    assert s.dtype == torch.float32 and tuple(s.shape) == ref_shape(mode, q.shape[0], p.shape[0], n), (mode, s.shape)
    s.backward(torch.from_numpy(np.asarray(G, np.float32)).cuda())
    grads = []
    for x, needed in ((tq, req[0]), (tp, req[1])):
        if not needed:
            assert x.grad is None
            grads.append(None)
            continue
        assert x.grad.dtype == tdt and tuple(x.grad.shape) == tuple(x.shape)
        grads.append(x.grad.float().cpu().numpy())
    return s.detach().cpu().numpy(), grads[0], grads[1]


@pytest.mark.gpu
def test_goldens_on_gpu_bit_equal():
    """scores, dq and dp of every fixture case, all three forms, fp32 and fp16 inputs, both sides and one side only: the same bits (an fp16
    gradient is the fixture's exact value rounded once to fp16)"""
    from dhr_amd import maxsim_scores as MS
    for key, z, q, p, n, mode in golden_cases():
        gq, gp = z[key + "_gq"] / 128.0, z[key + "_gp"] / 128.0
        for dtype in ("float32", "float16"):
            for req in ((True, True), (True, False), (False, True)):
                s, dq, dp = _run(MS, mode, q, p, n, z[key + "_G"], dtype, req)
                assert np.array_equal(s, z[key + "_scores"]), f"{key} {dtype} {req}: scores"
                for got, want, what in ((dq, gq, "dq"), (dp, gp, "dp")):
                    if got is None:
                        continue
                    want = want.astype(np.float16).astype(np.float32) if dtype == "float16" else want.astype(np.float32)
                    assert np.array_equal(got, want), f"{key} {dtype} {req}: {what}, {int((got != want).sum())} entries differ"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,grad", [("float32", "float16"), ("float16", "float32")])
def test_goldens_with_gradients_in_the_other_dtype(dtype, grad):
    """The torch wrapper asks for gradients in the dtype of the inputs; the library also writes fp16 gradients of fp32 inputs and fp32
    gradients of fp16 inputs.  The listwise fixture cases through the two entry points on host arrays: the same bits as above."""
    lib = _lib.load()
    code = {"float32": _lib.VAL_F32, "float16": _lib.VAL_F16}
    for key, z, q, p, n, mode in golden_cases():
        if mode != "list":
            continue
        (A, Lq, D), (B, Lp, _) = q.shape, p.shape
        hq, hp, G = (np.ascontiguousarray(x, dtype=d) for x, d in ((q, dtype), (p, dtype), (z[key + "_G"], np.float32)))
        out, arg = np.zeros((A, B), np.float32), np.zeros((A, B, Lq), np.int16)
        dq, dp = np.zeros((A, Lq, D), grad), np.zeros((B, Lp, D), grad)
        sides = (hq.ctypes.data, D, Lq * D, A, Lq, hp.ctypes.data, D, Lp * D, B, Lp, D, code[dtype], 0)
        assert lib.dhr_maxsim_scores(0, _lib.MEM_HOST, *sides, out.ctypes.data, B, arg.ctypes.data, None) == _lib.DHR_OK, lib.dhr_last_error()
        assert lib.dhr_maxsim_scores_backward(0, _lib.MEM_HOST, *sides, arg.ctypes.data, G.ctypes.data, B, dq.ctypes.data, dp.ctypes.data, code[grad],
                                              None) == _lib.DHR_OK, lib.dhr_last_error()
        assert np.array_equal(out, z[key + "_scores"]), f"{key} {dtype}: scores"
        for got, want, what in ((dq, z[key + "_gq"] / 128.0, "dq"), (dp, z[key + "_gp"] / 128.0, "dp")):
            assert np.array_equal(got.astype(np.float32), want.astype(grad).astype(np.float32)), f"{key} {dtype} -> {grad}: {what}"


# (A, B, Lq, Lp, D) -> the seed of each dtype, chosen on the CPU so that no winner is ambiguous and no fp16 gradient subnormal (both asserted
# below from the float64 restatement alone)
RANDOM_CASES = [((3, 8, 31, 149, 128), {"float16": 1, "float32": 1}),
                ((2, 4, 33, 65, 768), {"float16": 327, "float32": 0}),
                ((5, 5, 7, 300, 24), {"float16": 0, "float32": 0}),
                # ceil(A / 8) * B = 512 workgroups: two queries per wave, with D inside one 256-byte chunk of both dtypes, above one fp16 chunk
                # (128 columns) and above one fp32 chunk only (64 columns)
                ((64, 64, 2, 2, 8), {"float16": 0, "float32": 0}),
                ((64, 64, 2, 2, 130), {"float16": 1, "float32": 0}),
                ((64, 64, 2, 2, 66), {"float16": 1, "float32": 0})]


def _random_case(shape, dtype, seed):
    """continuous values: magnitudes uniform in [0.05, 1) (G: [0.25, 2)), random signs"""
    A, B, Lq, Lp, D = shape
    rng = np.random.default_rng([seed, A, B, D])
    cast = (lambda x: x.astype(np.float16).astype(np.float64)) if dtype == "float16" else (lambda x: x.astype(np.float32).astype(np.float64))
    draw = lambda lo, hi, size: rng.uniform(lo, hi, size) * rng.choice([-1.0, 1.0], size)  # noqa: E731
    return cast(draw(0.05, 1, (A, Lq, D))), cast(draw(0.05, 1, (B, Lp, D))), draw(0.25, 2, (A, B)).astype(np.float32)


def _unambiguous(t, pairs):
    return bool((t["gap"] > 2 * t["bsim"])[pairs].all())


def _fp16_normal(t):
    """The fp16 term of the tolerance, 2^-11 |truth|, is half an ulp only in fp16's normal range: no non-zero gradient may lie below 2^-14
    (a sum that cancels that far; the seeds avoid it, and this asserts it from the float64 truth alone)."""
    return all(bool((np.abs(t[k][t[k] != 0]) >= 2.0 ** -14).all()) for k in ("dq", "dp"))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,seeds", RANDOM_CASES)
def test_random_cases_against_restatement(shape, seeds):
    """Seeded continuous inputs, listwise and (where B is a multiple of A) pairwise: every entry of the scores and of both gradients inside
    the derived bound.  Nothing is left out: the seeds make every winner unambiguous."""
    from dhr_amd import maxsim_scores as MS
    A, B, Lq, Lp, D = shape
    for dtype in ("float16", "float32"):
        q, p, G = _random_case(shape, dtype, seeds[dtype])
        pairs = pairs_of("list", A, B, 0)
        t = truth(q, p, G.astype(np.float64), pairs)
        assert _unambiguous(t, pairs), f"{shape} {dtype}: an (a, b, i) of this seed has its two best similarities closer than twice the bound"
        assert dtype != "float16" or _fp16_normal(t), f"{shape}: a gradient entry of this seed is subnormal in fp16"
        s, dq, dp = _run(MS, "list", q, p, 0, G, dtype)
        what = f"random {shape} {dtype} list"
        assert_within(s, t["S"], t["bS"], what + " scores")
        assert_within(dq, t["dq"], t["bq"], what + " dq", fp16=dtype == "float16")
        assert_within(dp, t["dp"], t["bp"], what + " dp", fp16=dtype == "float16")
        if B % A == 0:
            n = B // A
            pairs = pairs_of("pair", A, B, n)
            Gn = G.reshape(-1)[:A * n].reshape(ref_shape("pair", A, B, n))
            t = truth(q, p, full_g(Gn, pairs), pairs)
            assert _unambiguous(t, pairs) and (dtype != "float16" or _fp16_normal(t))
            s, dq, dp = _run(MS, "pair", q, p, n, Gn, dtype)
            what = f"random {shape} {dtype} pair"
            assert_within(s, t["S"][pairs].reshape(Gn.shape), t["bS"][pairs].reshape(Gn.shape), what + " scores")
            assert_within(dq, t["dq"], t["bq"], what + " dq", fp16=dtype == "float16")
            assert_within(dp, t["dp"], t["bp"], what + " dp", fp16=dtype == "float16")


RECIPE_SEED = 0          # checked on the CPU: the restatement alone leaves no row out (the inputs are constructed for that, see the test)


def _recipe_inputs(A, B, Lq, Lp, D, seed):
    """fp16 token vectors with a planted match: every token carries small noise, D of the real tokens of passage b one large entry each, in
    a dimension of their own (a permutation of the D dimensions), every query token one large entry too.  Each (a, b, i) then has one
    passage token far ahead of the rest; the last 9 passage tokens are zero vectors (padding), as in the recipe.  The noise has magnitudes
    in [0.05, 0.25) and one sign per dimension, the large entries carry that sign, and G is in [0.25, 2): no gradient sum cancels, so
    none is subnormal in fp16 (asserted by the test), where 2^-11 |truth| would not be half an ulp.  -> (q, p, G) numpy"""
    rng = np.random.default_rng(seed)
    sign = rng.choice([-1.0, 1.0], D)
    q = rng.uniform(0.05, 0.25, (A, Lq, D))
    p = rng.uniform(0.05, 0.25, (B, Lp, D))
    real = Lp - 9
    k = min(real, D)
    dims = np.argsort(rng.random((B, D)), 1)[:, :k]
    toks = np.argsort(rng.random((B, real)), 1)[:, :k]
    p[np.arange(B)[:, None], toks, dims] += 3.0 + 3.0 * rng.random((B, k))
    p[:, real:] = 0
    q[np.arange(A)[:, None], np.arange(Lq)[None, :], rng.integers(0, D, (A, Lq))] += 4.0
    return (q * sign).astype(np.float16), (p * sign).astype(np.float16), rng.uniform(0.25, 2, (A, B)).astype(np.float32)


@pytest.mark.gpu
def test_recipe_sized_step_against_float64_on_the_device():
    """24 x 192, 31 x 149 tokens, D = 128, fp16: forward + backward against the restatement in torch float64 on the device, the same bounds.
    dq and dp are compared on the rows whose routed winners are all unambiguous; the share of the other rows is printed and stays below 1 %.
    The inputs are CONSTRUCTED, not merely seeded (_recipe_inputs): a planted match gives every (a, b, i) one passage token far ahead, so the
    share is zero by construction and the winner gaps are wider than in real data.  Plain continuous draws at this size cannot be used with
    these bounds: among 143 000 (a, b, i) about one in 2 500 has its two best similarities inside twice the similarity bound, which would
    leave some 7 % of the 744 dq rows out, and among 3 million fp16 gradient entries hundreds cancel into fp16's subnormal range, where
    2^-11 |truth| is not half an ulp.  Close winners are covered by the seeded continuous cases above, exact ties by the fixture."""
    import torch
    from dhr_amd import maxsim_scores as MS
    A, B, Lq, Lp, D = 24, 192, 31, 149, 128
    q16, p16, G = (torch.from_numpy(x).cuda() for x in _recipe_inputs(A, B, Lq, Lp, D, RECIPE_SEED))
    q, p, G64 = q16.double(), p16.double(), G.double()
    sim = torch.einsum("aik,bjk->abij", q, p)
    bsim = (D + 2) * U32 * torch.einsum("aik,bjk->abij", q.abs(), p.abs())
    top2, top2_j = sim.topk(2, dim=-1)
    arg = sim.argmax(-1)
    best = sim.gather(-1, arg[..., None])[..., 0]
    assert torch.equal(best, top2[..., 0])
    clear = (top2[..., 0] - top2[..., 1]) > 2 * bsim.amax(-1)                  # [A, B, Lq]
    S, bS = best.sum(-1), bsim.gather(-1, arg[..., None])[..., 0].sum(-1)
    won = torch.nn.functional.one_hot(arg, Lp).double()                        # [A, B, Lq, Lp]
    pw = p[None].expand(A, B, Lp, D).gather(2, arg[..., None].expand(A, B, Lq, D))
    dq = torch.einsum("ab,abid->aid", G64, pw)
    bq = (B + 2) * U32 * torch.einsum("ab,abid->aid", G64.abs(), pw.abs())
    dp = torch.einsum("ab,abij,aid->bjd", G64, won, q)
    bp = (won.sum((0, 2))[:, :, None] + 2) * U32 * torch.einsum("ab,abij,aid->bjd", G64.abs(), won, q.abs())
    # rows that an ambiguous winner could reach: the dq row of its (a, i), the dp rows of its two best tokens
    q_rows = clear.all(1)                                                      # [A, Lq]
    p_rows = torch.ones((B, Lp), dtype=torch.bool, device="cuda")
    amb = (~clear).nonzero()
    for k in range(2):
        p_rows[amb[:, 1], top2_j[amb[:, 0], amb[:, 1], amb[:, 2], k]] = False
    share_q, share_p = 1 - q_rows.double().mean().item(), 1 - p_rows.double().mean().item()
    print(f"recipe step: {int((~clear).sum())} of {clear.numel()} winners ambiguous; excluded rows: dq {100 * share_q:.3f} %, dp {100 * share_p:.3f} %")
    assert share_q < 0.01 and share_p < 0.01
    for x in (dq, dp):
        assert bool((x[x != 0].abs() >= 2.0 ** -14).all())                     # fp16's normal range: see _recipe_inputs

    tq, tp = q16.clone().requires_grad_(True), p16.clone().requires_grad_(True)
    s = MS.listwise_maxsim(tq, tp)
    s.backward(G)
    f = lambda x: x.double().cpu().numpy()  # noqa: E731
    assert_within(f(s.detach()), f(S), f(bS), "recipe scores")
    assert tq.grad.dtype == torch.float16 and tp.grad.dtype == torch.float16
    rq, rp = q_rows.cpu().numpy(), p_rows.cpu().numpy()
    assert_within(f(tq.grad)[rq], f(dq)[rq], f(bq)[rq], "recipe dq", fp16=True)
    assert_within(f(tp.grad)[rp], f(dp)[rp], f(bp)[rp], "recipe dp", fp16=True)


class _Spy:
    """the loaded library with the two maxsim entry points recorded"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("dhr_maxsim"):
            return fn

        def recorded(*args):
            self.calls.append((name, args))
            return fn(*args)
        return recorded


@pytest.mark.gpu
def test_views_are_read_in_place(monkeypatch):
    """reps[:, 1:] of [A, L, D] tensors on both sides: the library gets the views' own pointers and strides (no hidden .contiguous()), the
    gradient arrives in the base tensors' .grad with zeros at token 0."""
    import torch
    from dhr_amd import maxsim_scores as MS
    A, B, Lq, Lp, D = 3, 6, 9, 20, 128
    rng = np.random.default_rng(3)
    q8, p8 = rng.integers(-16, 17, (A, Lq + 1, D)), rng.integers(-16, 17, (B, Lp + 1, D))
    G = (rng.integers(-32, 33, (A, B)) / 16.0)
    spy = _Spy(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: spy)
    for dtype in (torch.float16, torch.float32):
        spy.calls.clear()
        bq = torch.from_numpy(q8 / 8.0).to("cuda", dtype).requires_grad_(True)
        bp = torch.from_numpy(p8 / 8.0).to("cuda", dtype).requires_grad_(True)
        vq, vp = bq[:, 1:], bp[:, 1:]
        assert not vq.is_contiguous() and vq.data_ptr() != bq.data_ptr()
        s = MS.listwise_maxsim(vq, vp)
        s.backward(torch.from_numpy(G).float().cuda())
        assert [c[0] for c in spy.calls] == ["dhr_maxsim_scores", "dhr_maxsim_scores_backward"]
        for name, a in spy.calls:
            # (device, mem_kind, q, ld_q_tok, ld_q_batch, A, Lq, p, ld_p_tok, ld_p_batch, B, Lp, D, ...)
            assert a[1] == _lib.MEM_DEVICE and a[2:7] == (vq.data_ptr(), D, (Lq + 1) * D, A, Lq) and a[7:13] == (vp.data_ptr(), D, (Lp + 1) * D, B, Lp, D), name
        pairs = pairs_of("list", A, B, 0)
        t = truth(q8[:, 1:] / 8.0, p8[:, 1:] / 8.0, G, pairs)
        assert np.array_equal(s.detach().cpu().numpy(), t["S"].astype(np.float32))
        for base, want in ((bq, t["dq"]), (bp, t["dp"])):
            g = base.grad
            assert g.dtype == dtype and tuple(g.shape) == tuple(base.shape) and not g[:, 0].any()
            assert np.array_equal(g[:, 1:].float().cpu().numpy(), want.astype(np.float16 if dtype == torch.float16 else np.float32).astype(np.float32))


@pytest.mark.gpu
def test_runs_are_bit_identical_and_forms_agree(monkeypatch):
    """Two runs: the same bits.  group = n: the matching block of group = 0, bit for bit (two queries per wave in one, one in the other).
    torch.no_grad(): the same scores, and no winners are allocated or stored."""
    import torch
    from dhr_amd import maxsim_scores as MS
    rng = np.random.default_rng(17)
    for (A, n, Lq, Lp, D), dtype in (((40, 16, 31, 149, 128), torch.float16), ((6, 3, 33, 65, 200), torch.float32), ((5, 1, 7, 40, 20), torch.float16)):
        B = A * n
        q = torch.from_numpy(rng.uniform(-1, 1, (A, Lq, D))).to("cuda", dtype)
        p = torch.from_numpy(rng.uniform(-1, 1, (B, Lp, D))).to("cuda", dtype)
        G = torch.from_numpy(rng.uniform(-2, 2, (A, B))).float().cuda()
        runs = []
        for _ in range(2):
            tq, tp = q.clone().requires_grad_(True), p.clone().requires_grad_(True)
            s = MS.maxsim_scores(tq, tp)
            s.backward(G)
            runs.append((s.detach(), tq.grad, tp.grad))
        for a, b in zip(*runs):
            assert torch.equal(a, b)
        own = torch.arange(A, device="cuda")[:, None] * n + torch.arange(n, device="cuda")[None, :]
        tq, tp = q.clone().requires_grad_(True), p.clone().requires_grad_(True)
        sn = MS.maxsim_scores(tq, tp, group=n)
        assert tuple(sn.shape) == (A, n) and torch.equal(sn.detach(), runs[0][0].gather(1, own))
        # no gradient to compute: the same scores, arg == NULL at the library and no int16 tensor made
        spy = _Spy(_lib.load())
        monkeypatch.setattr(_lib, "load", lambda: spy)
        made = []
        real_empty = _marshal.empty
        monkeypatch.setattr(_marshal, "empty", lambda like, shape, name: made.append(name) or real_empty(like, shape, name))
        with torch.no_grad():
            s0 = MS.maxsim_scores(tq, tp)
        s1 = MS.maxsim_scores(q, p)
        monkeypatch.undo()
        assert torch.equal(s0, runs[0][0]) and torch.equal(s1, runs[0][0]) and not s0.requires_grad
        assert [c[0] for c in spy.calls] == ["dhr_maxsim_scores"] * 2 and all(c[1][17] is None for c in spy.calls) and made == ["float32"] * 2


@pytest.mark.gpu
def test_memory_stays_far_below_the_similarity_tensor():
    """(8, 64, 31, 149, 128) fp16: the peak over forward + backward, minus what was allocated before the call and minus the returned tensors
    (scores and the two .grad), stays below a quarter of the bytes of ONE fp32 [A, B, Lq, Lp] tensor."""
    import torch
    from dhr_amd import maxsim_scores as MS
    A, B, Lq, Lp, D = 8, 64, 31, 149, 128
    gen = torch.Generator(device="cuda").manual_seed(3)
    q = (torch.rand((A, Lq, D), device="cuda", generator=gen) - 0.5).half().requires_grad_(True)
    p = (torch.rand((B, Lp, D), device="cuda", generator=gen) - 0.5).half().requires_grad_(True)
    G = torch.rand((A, B), device="cuda", generator=gen)
    MS.listwise_maxsim(q, p).backward(G)                          # warm-up: the library is loaded, kernels are resident
    q.grad = p.grad = None
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    s = MS.listwise_maxsim(q, p)
    s.backward(G)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    returned = sum(t.numel() * t.element_size() for t in (s, q.grad, p.grad))
    extra, limit = peak - before - returned, A * B * Lq * Lp * 4 // 4
    print(f"memory: peak {peak - before} B over the call, returned tensors {returned} B, the op's own {extra} B; limit {limit} B")
    assert extra < limit


def _eager(q, p):
    """the reference's op sequence (modeling.py:216-218)"""
    import torch
    scores = torch.einsum("aik,bjk->abij", q, p)
    return torch.sum(torch.max(scores, -1).values, -1)


@pytest.mark.gpu
def test_timing_printout():
    """Forward + backward at the recipe's shapes, fp16, this library against the eager composition of the reference's ops, alternating:
    device events around windows of iterations after a warm-up, three repeats so the spread shows.  A printout, never a threshold."""
    import torch
    from dhr_amd import maxsim_scores as MS
    Lq, Lp, D = 31, 149, 128
    for A, B, iters in ((24, 192, 20), (96, 768, 10), (192, 1536, 5)):
        gen = torch.Generator(device="cuda").manual_seed(A)
        q = (torch.rand((A, Lq, D), device="cuda", generator=gen) - 0.5).half().requires_grad_(True)
        p = (torch.rand((B, Lp, D), device="cuda", generator=gen) - 0.5).half().requires_grad_(True)
        G = torch.randn((A, B), device="cuda", generator=gen)

        def step(fn):
            q.grad = p.grad = None
            s = fn(q, p)
            s.backward(G.to(s.dtype))

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
            for name, fn in (("fused", MS.listwise_maxsim), ("eager", _eager)):
                window(fn, 2)
                times[name].append(window(fn, iters))
                q.grad = p.grad = None
                torch.cuda.empty_cache()                          # the eager side keeps several GB at the largest shape
        f, e = times["fused"], times["eager"]
        print(f"maxsim fwd+bwd A={A} B={B} {Lq}x{Lp} tokens D={D} fp16: fused " + " / ".join(f"{t:.3f}" for t in f) + " ms, eager torch " +
              " / ".join(f"{t:.3f}" for t in e) + f" ms, {np.median(e) / np.median(f):.1f}x")
        del q, p, G
        torch.cuda.empty_cache()


@pytest.mark.gpu
def test_host_arrays_with_strides_match_the_device_path():
    """A = 2, B = 3, Lq = 2, Lp = 3, D = 5 as base[:, 1:, :5] of bases with D padded to 8, scores and the upstream gradient in wider rows:
    both entry points on host pointers (staged through the device, complete on return) give the bits of the same views on the device."""
    import torch
    from dhr_amd import maxsim_scores as MS
    lib = _lib.load()
    A, B, Lq, Lp, D = 2, 3, 2, 3, 5
    rng = np.random.default_rng(9)
    bq, bp = rng.uniform(-1, 1, (A, Lq + 1, 8)).astype(np.float32), rng.uniform(-1, 1, (B, Lp + 1, 8)).astype(np.float32)
    bG = rng.uniform(-1, 1, (A, B + 2)).astype(np.float32)
    out, arg = np.full((A, B + 1), 7, np.float32), np.zeros((A, B, Lq), np.int16)
    dq, dp = np.zeros((A, Lq, D), np.float32), np.zeros((B, Lp, D), np.float32)
    sides = (bq[:, 1:].ctypes.data, 8, (Lq + 1) * 8, A, Lq, bp[:, 1:].ctypes.data, 8, (Lp + 1) * 8, B, Lp, D, _lib.VAL_F32, 0)
    assert lib.dhr_maxsim_scores(0, _lib.MEM_HOST, *sides, out.ctypes.data, B + 1, arg.ctypes.data, None) == _lib.DHR_OK, lib.dhr_last_error()
    assert lib.dhr_maxsim_scores_backward(0, _lib.MEM_HOST, *sides, arg.ctypes.data, bG.ctypes.data, B + 2, dq.ctypes.data, dp.ctypes.data, _lib.VAL_F32,
                                          None) == _lib.DHR_OK, lib.dhr_last_error()
    tq, tp = (torch.from_numpy(b).cuda()[:, 1:, :D].requires_grad_(True) for b in (bq, bp))
    s = MS.maxsim_scores(tq, tp)
    s.backward(torch.from_numpy(bG).cuda()[:, :B])
    assert np.array_equal(out[:, :B], s.detach().cpu().numpy()) and (out[:, B:] == 7).all()
    assert np.array_equal(dq, tq.grad.cpu().numpy()) and np.array_equal(dp, tp.grad.cpu().numpy())
    assert np.array_equal(MS.maxsim_scores(bq[:, 1:, :D], bp[:, 1:, :D]), out[:, :B])          # numpy in -> numpy out, the same bits
