"""The fused training loss (dhr_amd/train_loss.py on dhr_train_loss): hybrid KL / contrastive loss with its gradients.

Truth is the float64 restatement below (`truth`).  The tolerance is derived, not measured.  With u = 2^-24, per term k with student scores s
and scaled teacher t, d(x) = |x - rowmax(x)|:
    loss      w_k / R * u * sum_{r,c} P * ((C + 8) * (|log P| + |log_softmax s|) + 4 * (d(s) + d(t) + |s| + |t|)), summed over the terms
    gradient  w_k / R * (u * ((C + 8 + 2 d(s) + 2 |s|) * softmax(s) + (C + 8 + 2 d(t) + 2 |t|) * P) + 2^-126) per entry, summed over the terms
              that reach the input (the fused term reaches semantic with factor lamb), plus 4 u |truth|; with hard labels P is exact and its
              part drops; fp16 outputs add 2^-11 |truth|; the 2^-126 floor covers targets and softmax entries that underflow
    scores    2 u |truth| (one rounding of the fused multiply-add)
The golden fixture (the reference's own forwards, tests/golden/make_golden_train_loss.py) is the reference's fp32 result: it lies within the
same bounds of the restatement, and so must the library.

CPU part (-m "not gpu"): the fixture against the restatement, statuses of the entry point on host pointers, the wrappers' errors, the names.
GPU part: goldens, seeded cases at the smallest shapes that can go wrong, a recipe-sized step, bit-identity, upstream scaling, memory, stream
order, and a timing comparison with the eager composition of the reference's ops.

Measured on an MI355X (profiles/train_loss.txt): fused 0.13 ms against eager 0.43 ms per step at (24, 192), 0.08 against 0.37 ms at
(192, 1536); worst error / bound: loss 0.07, fp32 gradients 0.57, fp16 gradients 0.97, scores 0.50."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

from dhr_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "train_loss_golden.npz")
U, U16, TINY = 2.0 ** -24, 2.0 ** -11, 2.0 ** -126
DHR_W, HARD_W, SPLIT = (1.0, 0.5, 0.5), (1.0, 0.0, 0.0), (1.0, 0.75, 0.25)
NEW = ("dhr_train_loss_workspace", "dhr_train_loss")


# ------------------------------------------------------------------------------------------ float64 restatement
def _log_softmax(x):
    d = x - x.max(1, keepdims=True)
    return d - np.log(np.exp(d).sum(1, keepdims=True)), np.abs(d)


def truth(lex, sem, tea, n, lamb=1.0, temperature=1.0, weights=DHR_W, split=SPLIT):
    """float64 [R, C] matrices (sem / tea may be None) -> dict: loss, b_loss; scores; g_lex, b_lex; g_sem, b_sem (None without sem).
    b_* are the bounds of the module docstring without the fp16 term."""
    R, Cn = lex.shape
    fused = lex + lamb * sem if sem is not None else lex
    students = (fused, sem, lex)
    loss = b_loss = 0.0
    g = [np.zeros((R, Cn)), np.zeros((R, Cn))]          # lexical, semantic
    b = [np.zeros((R, Cn)), np.zeros((R, Cn))]
    for k in range(3):
        w = float(weights[k])
        if w == 0.0:
            continue
        s = students[k]
        lsm, ds = _log_softmax(s)
        q = np.exp(lsm)
        if tea is not None:
            t = tea * temperature * split[k]
            logp, dt = _log_softmax(t)
            P = np.exp(logp)
            bP = (Cn + 8 + 2 * dt + 2 * np.abs(t)) * P
        else:
            P = np.zeros((R, Cn))
            P[np.arange(R), np.arange(R) * n] = 1.0
            t = dt = logp = bP = np.zeros((R, Cn))         # P is exact: its part of the bounds drops
        loss += w / R * np.where(P > 0, P * (logp - lsm), 0.0).sum()
        b_loss += abs(w) / R * U * (P * ((Cn + 8) * (np.abs(logp) + np.abs(lsm)) + 4 * (ds + dt + np.abs(s) + np.abs(t)))).sum()
        gk = w / R * (q - P)
        bk = abs(w) / R * (U * ((Cn + 8 + 2 * ds + 2 * np.abs(s)) * q + bP) + TINY)
        for side, factor in {0: ((0, 1.0), (1, lamb)), 1: ((1, 1.0),), 2: ((0, 1.0),)}[k]:
            g[side] += factor * gk
            b[side] += abs(factor) * bk
    out = dict(loss=loss, b_loss=b_loss, scores=fused, g_lex=g[0], b_lex=b[0] + 4 * U * np.abs(g[0]), g_sem=None, b_sem=None)
    if sem is not None:
        out.update(g_sem=g[1], b_sem=b[1] + 4 * U * np.abs(g[1]))
    return out


def assert_within(got, want, bound, what, fp16=False):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    tol = np.asarray(bound, np.float64) + (U16 * np.abs(want) if fp16 else 0.0)
    err = np.abs(got - want)
    worst = float((err / np.where(tol > 0, tol, 1.0))[tol > 0].max()) if (tol > 0).any() else 0.0
    print(f"{what}: max error / bound = {worst:.4f}")
    assert not (err > tol).any(), f"{what}: {int((err > tol).sum())} of {err.size} entries outside the bound (worst error / bound {worst:.3f})"


def golden_cases():
    z = np.load(GOLDEN)
    for name in z["names"]:
        cfg = z[name + "_cfg"]
        get = lambda k: z[name + k] if name + k in z.files else None   # noqa: E731
        yield str(name), z, dict(lex=z[name + "_lex"], sem=get("_sem"), tea=get("_teacher"), n=int(cfg[1]), lamb=float(cfg[2]),
                                 temperature=float(cfg[3]), weights=tuple(cfg[4:7]), split=tuple(cfg[7:10]))


def _truth_of(c):
    f = lambda a: None if a is None else a.astype(np.float64)   # noqa: E731
    return truth(f(c["lex"]), f(c["sem"]), f(c["tea"]), c["n"], c["lamb"], c["temperature"], c["weights"], c["split"])


# ------------------------------------------------------------------------------------------ CPU part
def test_fixture_matches_float64_restatement():
    seen = set()
    for name, z, c in golden_cases():
        t = _truth_of(c)
        R, n = int(z[name + "_cfg"][0]), c["n"]
        assert c["lex"].shape == (R, R * n) and c["lex"].dtype == np.float32
        for m in (c["lex"], c["sem"], c["tea"]):
            assert m is None or np.array_equal(m * 8, np.rint(m * 8))               # multiples of 2^-3: the score matrices are exact
        assert_within(z[name + "_loss"], t["loss"], t["b_loss"], name + " loss")
        assert_within(z[name + "_scores"], t["scores"], 2 * U * np.abs(t["scores"]), name + " scores")
        assert_within(z[name + "_glex"], t["g_lex"], t["b_lex"], name + " dlexical")
        if c["sem"] is not None:
            assert_within(z[name + "_gsem"], t["g_sem"], t["b_sem"], name + " dsemantic")
        seen.add(name.rsplit("_", 1)[0])
    kinds = {"dhr_tct", "dhr_tct_half", "dhr_hard", "agg_tct", "agg_hard_sem", "agg_hard_nosem", "dense_ce", "colbert_kd"}
    assert kinds == seen and len(z["names"]) == 3 * len(kinds)
    assert {tuple(int(v) for v in z[k + "_cfg"][:2]) for k in z["names"]} == {(2, 3), (3, 1), (8, 4)}
    assert "agg_hard_nosem_2x3_sem" not in z.files and (z["colbert_kd_8x4_teacher"] == -20).any() and os.path.getsize(GOLDEN) < 256 * 1024
    assert tuple(z["dhr_tct_half_2x3_cfg"][2:4]) == (0.5, 0.5) and tuple(z["agg_hard_sem_2x3_cfg"][4:7]) == DHR_W


_H = {k: np.zeros((2, 6), np.float32) for k in ("lex", "sem", "tea", "scores", "gl", "gs")}
_H["loss"] = np.zeros(1, np.float32)


def _call(lib, **kw):
    """dhr_train_loss on valid host arguments (2 queries x 6 passages, three fp32 matrices, every output), with overrides"""
    p = lambda k: _H[k].ctypes.data   # noqa: E731
    a = dict(device=0, mem_kind=_lib.MEM_HOST, lexical=p("lex"), lexical_dtype=_lib.VAL_F32, ld_lexical=6, semantic=p("sem"), semantic_dtype=_lib.VAL_F32,
             ld_semantic=6, teacher=p("tea"), teacher_dtype=_lib.VAL_F32, ld_teacher=6, rows=2, cols=6, label_stride=3, lamb=1.0, temperature=1.0,
             weights=DHR_W, split=SPLIT, loss=p("loss"), scores=p("scores"), ld_scores=6, gl=p("gl"), ld_gl=6, gs=p("gs"), ld_gs=6, ws=None, ws_bytes=0,
             stream=None)
    assert set(kw) <= set(a), kw
    a.update(kw)
    for k in ("weights", "split"):
        a[k] = None if a[k] is None else (C.c_float * 3)(*a[k])
    return lib.dhr_train_loss(*a.values())


def test_entry_point_returns_statuses():
    import torch
    lib = _lib.load()
    assert lib.dhr_version() == 105
    assert lib.dhr_train_loss_workspace(24) == 96 and lib.dhr_train_loss_workspace(0) == 0 and lib.dhr_train_loss_workspace(-3) == 0
    invalid = [dict(lexical=None), dict(loss=None), dict(weights=None), dict(rows=-1), dict(cols=-1), dict(mem_kind=7), dict(mem_kind=-1),
               dict(lexical_dtype=5), dict(semantic_dtype=-1), dict(teacher_dtype=2), dict(ld_lexical=5), dict(ld_semantic=0), dict(ld_teacher=-6),
               dict(ld_scores=5), dict(ld_gl=5), dict(ld_gs=5),
               # a teacher needs positive scales: the three targets share its row maximum
               dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(split=(1.0, 0.0, 0.25)), dict(split=(-1.0, 0.75, 0.25)),
               dict(split=(1.0, 0.75, -0.25)), dict(split=None),
               # hard labels: the label of the last row must be a column
               dict(teacher=None, label_stride=6), dict(teacher=None, label_stride=7), dict(teacher=None, label_stride=-1),
               dict(teacher=None, rows=1, cols=0 + 6, label_stride=-2),
               # no semantic scores: no semantic term, no semantic gradient
               dict(semantic=None, gs=None), dict(semantic=None, gs=None, weights=(0.0, 0.25, 0.0)), dict(semantic=None, weights=HARD_W),
               # device arrays need the workspace
               dict(mem_kind=_lib.MEM_DEVICE), dict(mem_kind=_lib.MEM_DEVICE, ws=_H["gl"].ctypes.data, ws_bytes=7)]
    for b in invalid:
        _H["loss"][0] = 7.0
        assert _call(lib, **b) == _lib.ERR_INVALID and lib.dhr_last_error(), b
        assert _H["loss"][0] == 7.0
    assert _call(lib, teacher=None, label_stride=6) == _lib.ERR_INVALID and b"label column" in lib.dhr_last_error()
    assert _call(lib, semantic=None, gs=None) == _lib.ERR_INVALID and b"semantic" in lib.dhr_last_error()
    assert _call(lib, cols=(1 << 30) + 1, ld_lexical=1 << 31, ld_semantic=1 << 31, ld_teacher=1 << 31, ld_scores=1 << 31, ld_gl=1 << 31,
                 ld_gs=1 << 31) == _lib.ERR_UNSUPPORTED
    # nothing to do: loss 0, nothing else is touched, no device
    for b in (dict(rows=0), dict(cols=0, ld_lexical=0, ld_semantic=0, ld_teacher=0), dict(rows=0, teacher=None, label_stride=100)):
        _H["loss"][0] = 7.0
        _H["scores"][:] = 3.0
        assert _call(lib, **b) == _lib.DHR_OK and _H["loss"][0] == 0.0 and (_H["scores"] == 3.0).all(), b
    # valid calls: a status without a device, the result with one
    valid = [dict(), dict(teacher=None), dict(teacher=None, label_stride=5), dict(teacher=None, temperature=0.0, split=None),
             dict(semantic=None, gs=None, weights=(1.0, 0.0, 0.5)), dict(scores=None, gl=None, gs=None), dict(weights=(0.0, 0.0, 0.0))]
    want = _lib.DHR_OK if torch.cuda.is_available() else _lib.ERR_HIP
    rcs = [_call(lib, **b) for b in valid]
    assert all(rc == want for rc in rcs), rcs
    if torch.cuda.is_available():                       # all-zero scores, DHR weights with a teacher: every KL term is 0, softmax uniform
        assert _call(lib) == _lib.DHR_OK and _H["loss"][0] == 0.0 and not _H["gl"].any() and not _H["scores"].any()
        assert _call(lib, teacher=None) == _lib.DHR_OK and abs(_H["loss"][0] - 2 * np.log(6.0)) < 1e-5
    else:
        from dhr_amd import train_loss as TL
        with pytest.raises(_lib.DhrError, match="dhr_train_loss failed"):
            TL.contrastive_loss(torch.zeros(2, 6), 3)


def test_wrappers_raise_before_touching_the_library(monkeypatch):
    import torch
    from dhr_amd import train_loss as TL

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    z = lambda *s, **kw: torch.zeros(*s, **kw)   # noqa: E731
    for grad in (False, True):
        lex = z(2, 6, requires_grad=grad)
        with pytest.raises(RuntimeError, match=r"semantic_scores \(2, 5\) do not match lexical_scores \(2, 6\)"):
            TL.dhr_loss(lex, z(2, 5), train_n_passages=3, lamb=1.0)
        with pytest.raises(RuntimeError, match=r"teacher_scores \(3, 6\) do not match"):
            TL.dhr_loss(lex, z(2, 6), z(3, 6), train_n_passages=3, lamb=1.0)
        with pytest.raises(RuntimeError, match="teacher_scores"):
            TL.distill_loss(lex, z(2, 3))
        with pytest.raises(ValueError, match=r"\[queries, passages\]"):
            TL.contrastive_loss(z(2, 3, 2), 1)
        with pytest.raises(ValueError, match=r"\[queries, passages\]"):
            TL.hybrid_loss(lex, z(12), train_n_passages=3)
        # a label outside the columns (the reference: RuntimeError from one_hot)
        with pytest.raises(RuntimeError, match="train_n_passages = 6 puts the label of query 1 at column 6, outside 6 passages"):
            TL.contrastive_loss(lex, 6)
        with pytest.raises(RuntimeError, match="outside 6 passages"):
            TL.dhr_loss(lex, z(2, 6), train_n_passages=7, lamb=1.0)
        with pytest.raises(RuntimeError, match="outside 6 passages"):
            TL.aggretriever_loss(lex, train_n_passages=-1)
        with pytest.raises(ValueError, match="no semantic scores"):
            TL.hybrid_loss(lex, train_n_passages=3)                                   # the default weights have a semantic term
        with pytest.raises(ValueError, match="semantic"):
            TL.dhr_loss(lex, None, train_n_passages=3, lamb=1.0)
        with pytest.raises(ValueError, match="need semantic scores"):
            TL.aggretriever_loss(lex, None, z(2, 6), train_n_passages=3)
        for bad in (dict(temperature=0.0), dict(temperature=-2.0), dict(teacher_split=(1.0, 0.0, 0.25))):
            with pytest.raises(ValueError, match="must be positive"):
                TL.hybrid_loss(lex, z(2, 6), z(2, 6), train_n_passages=3, **bad)
        with pytest.raises(ValueError, match="three values"):
            TL.hybrid_loss(lex, z(2, 6), train_n_passages=3, weights=(1.0, 0.5))
        with pytest.raises(TypeError, match="torch tensor"):
            TL.hybrid_loss(lex, np.zeros((2, 6), np.float32), train_n_passages=3)
        with pytest.raises(_lib.DhrError, match="one device"):
            TL.dhr_loss(lex, z(2, 6, device="meta"), train_n_passages=3, lamb=1.0)
        with pytest.raises(_lib.DhrError, match="one device"):
            TL.distill_loss(lex, z(2, 6, device="meta"))


def test_new_symbols_are_declared_mapped_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "dhr_hip.h")).read()
    vmap = open(os.path.join(ROOT, "dhr_amd", "csrc", "libdhr.map")).read()
    globs = re.findall(r"^\s*([a-z_*]+);", vmap.split("local:")[0], re.M)
    lib = _lib.load()
    for name in NEW:
        assert name + "(" in header and name in _lib.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
        assert any(fnmatch.fnmatch(name, p) for p in globs), globs
    m = re.search(r"^int\s+dhr_train_loss\s*\(([^;]*?)\)\s*;", header, re.S | re.M)
    assert m and " ".join(m.group(1).split(",")[-1].split()) == "void* stream" and len(m.group(1).split(",")) == len(lib.dhr_train_loss.argtypes)
    assert lib.dhr_version() == 105
    from dhr_amd import _build
    assert "train_loss.hip" in _build.SOURCES
    from dhr_amd import train_loss as TL
    for fn in ("hybrid_loss", "dhr_loss", "aggretriever_loss", "contrastive_loss", "distill_loss"):
        assert callable(getattr(TL, fn))


# ------------------------------------------------------------------------------------------ GPU part
def _cast64(a, dtype):
    return None if a is None else np.asarray(a).astype(dtype).astype(np.float64)


def _dev(a, dtype, grad=False):
    import torch
    return None if a is None else torch.from_numpy(np.asarray(a, np.float64)).to("cuda", getattr(torch, dtype)).requires_grad_(grad)


def _run(lex, sem, tea, n, lamb=1.0, temperature=1.0, weights=DHR_W, split=SPLIT, dtypes=("float32",) * 3, req=(True, True), view=False):
    """One call on device tensors made from float64 arrays that the dtypes hold exactly.  view: the matrices are [:, 1:] views of wider ones.
    -> (loss, scores, dlexical or None, dsemantic or None) as numpy, gradients as float32 with the tensors' dtype checked"""
    import torch
    from dhr_amd import train_loss as TL

    def make(a, dtype, grad):
        if a is None:
            return None, None
        if not view:
            t = _dev(a, dtype, grad)
            return t, t
        base = _dev(np.concatenate([np.full((a.shape[0], 1), 77.0), a], 1), dtype, grad)
        v = base[:, 1:]
        assert not v.is_contiguous() or a.shape[0] == 1
        return base, v
    bl, tl = make(lex, dtypes[0], req[0])
    bs, ts = make(sem, dtypes[1], req[1] and sem is not None)
    _, tt = make(tea, dtypes[2], False)
    loss, scores = TL.hybrid_loss(tl, ts, tt, train_n_passages=n if n is not None else 1, lamb=lamb, temperature=temperature, weights=weights,
                                  teacher_split=split)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and scores.dtype == torch.float32 and tuple(scores.shape) == lex.shape
    assert not scores.requires_grad
    needs = req[0] or (req[1] and sem is not None)
    assert loss.requires_grad == needs
    if needs:
        loss.backward()
    grads = []
    for base, a, dtype, need in ((bl, lex, dtypes[0], req[0]), (bs, sem, dtypes[1], req[1])):
        if base is None or not need:
            assert base is None or base.grad is None
            grads.append(None)
            continue
        assert base.grad.dtype == getattr(torch, dtype) and base.grad.shape == base.shape
        g = base.grad.float().cpu().numpy()
        if view:
            assert not g[:, 0].any()
            g = g[:, 1:]
        grads.append(g)
    return float(loss.item()), scores.cpu().numpy(), grads[0], grads[1]


def _check(got, t, what, dtypes=("float32",) * 3):
    loss, scores, gl, gs = got
    assert_within(loss, t["loss"], t["b_loss"], what + " loss")
    assert_within(scores, t["scores"], 2 * U * np.abs(t["scores"]), what + " scores")
    if gl is not None:
        assert_within(gl, t["g_lex"], t["b_lex"], what + " dlexical", fp16=dtypes[0] == "float16")
    if gs is not None:
        assert_within(gs, t["g_sem"], t["b_sem"], what + " dsemantic", fp16=dtypes[1] == "float16")


@pytest.mark.gpu
def test_goldens_on_gpu():
    """every fixture case within the bound of the restatement, every combination of gradients.  fp16 inputs (the fixture's values are exact in
    fp16 too) are checked on the loss and the scores: the fixture's small softmax entries give gradients below fp16's normal range, where
    2^-11 |truth| is not half an ulp (fp16 gradients: test_mixed_dtypes_views_and_lamb)."""
    for name, z, c in golden_cases():
        t = _truth_of(c)
        for req in ((True, True), (True, False), (False, True)):
            _check(_run(c["lex"], c["sem"], c["tea"], c["n"], c["lamb"], c["temperature"], c["weights"], c["split"], req=req), t, f"golden {name} {req}")
        _check(_run(c["lex"], c["sem"], c["tea"], c["n"], c["lamb"], c["temperature"], c["weights"], c["split"], dtypes=("float16",) * 3,
                    req=(False, False)), t, f"golden {name} float16")


def _seeded(R, Cn, seed, scale=2.0, dtypes=("float32",) * 3):
    """-> (lex, sem, tea) float64 arrays that `dtypes` hold exactly"""
    rng = np.random.default_rng([seed, R, Cn])
    return tuple(_cast64(rng.normal(0.0, scale, (R, Cn)), dt) for dt in dtypes)


# (R, C, train_n_passages or None: teacher only): (1, 1, 1) must give exact zeros; below, at and above one pass of 256 lanes (a thread takes 4
# columns, so 1025 and 4097 are one column past a whole pass of 1024 and four of them: the vector-load tail); the recipe's (24, 192, 8)
SEEDED = [(1, 1, 1), (2, 6, 3), (3, 7, None), (5, 255, 51), (4, 256, 64), (3, 257, None), (2, 1025, None), (2, 4097, None), (24, 192, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("R,Cn,n", SEEDED)
def test_seeded_cases_against_restatement(R, Cn, n):
    """with and without a teacher; both gradients, one of them, none"""
    lex, sem, tea = _seeded(R, Cn, 1)
    for teacher in ((True, False) if n is not None else (True,)):
        t = truth(lex, sem, tea if teacher else None, n, 1.0, 1.0, DHR_W, SPLIT)
        for req in ((True, True), (True, False), (False, True), (False, False)):
            got = _run(lex, sem, tea if teacher else None, n, req=req)
            _check(got, t, f"seeded {R}x{Cn} teacher={teacher} grads={req}")
            if (R, Cn) == (1, 1):
                assert got[0] == 0.0 and all(g is None or not g.any() for g in got[2:]), got


def _clustered(R, Cn, seed, dtypes):
    """Inputs whose fp16 gradients stay in fp16's normal range, where the fp16 term of the tolerance, 2^-11 |truth|, is half an ulp: every
    entry of the two students is +-(0.5 + noise) with one random sign per entry, shared by both, and the teacher is -+(1 + noise).  Every
    softmax(s) - P then has the entry's sign in all three terms, so no gradient sum cancels, and its size is of the order 1 / C.
    -> (lex, sem, tea) float64 arrays that `dtypes` hold exactly"""
    rng = np.random.default_rng([seed, R, Cn])
    sign = rng.choice([-1.0, 1.0], (R, Cn))
    mag = lambda: 1.0 + rng.uniform(-0.25, 0.25, (R, Cn))   # noqa: E731
    return tuple(_cast64(f * sign * mag(), dt) for f, dt in zip((0.5, 0.5, -1.0), dtypes))


def _fp16_normal(t):
    return all(t[k] is None or bool((np.abs(t[k][t[k] != 0]) >= 2.0 ** -14).all()) for k in ("g_lex", "g_sem"))


MIXED_SHAPES = ((5, 255, 51), (4, 256, 64), (2, 1025, 2))
MIXED_DTYPES = (("float32", "float16", "float16"), ("float16",) * 3, ("float32",) * 3)


def test_fp16_gradient_cases_stay_in_the_normal_range():
    """from the float64 restatement alone: no gradient entry of the mixed-dtype cases is below 2^-14"""
    for R, Cn, n in MIXED_SHAPES:
        for dtypes in MIXED_DTYPES:
            lex, sem, tea = _clustered(R, Cn, 2, dtypes)
            for teacher in (tea, None):
                assert _fp16_normal(truth(lex, sem, teacher, n)), (R, Cn, dtypes, teacher is None)


@pytest.mark.gpu
def test_mixed_dtypes_views_and_lamb():
    """fp32 lexical with fp16 semantic and teacher, all fp16, all fp32; packed and as [:, 1:] views of wider matrices (ld > C and a base
    pointer off 16 bytes: the element-wise loads beside the vector ones of the packed case); then lamb of 0 and of 0.5 with a temperature of
    0.5, and no semantic scores"""
    for R, Cn, n in MIXED_SHAPES:
        for dtypes in MIXED_DTYPES:
            lex, sem, tea = _clustered(R, Cn, 2, dtypes)
            for view in (False, True):
                for teacher in (True, False):
                    t = truth(lex, sem, tea if teacher else None, n)
                    _check(_run(lex, sem, tea if teacher else None, n, dtypes=dtypes, view=view), t, f"{R}x{Cn} {dtypes} view={view} teacher={teacher}",
                           dtypes)
    lex, sem, tea = _seeded(5, 255, 3)
    for lamb in (0.0, 0.5):
        for teacher in (True, False):
            t = truth(lex, sem, tea if teacher else None, 51, lamb=lamb, temperature=0.5)
            got = _run(lex, sem, tea if teacher else None, 51, lamb=lamb, temperature=0.5)
            _check(got, t, f"lamb={lamb} teacher={teacher}")
            if lamb == 0.0:
                assert np.array_equal(got[1], lex.astype(np.float32))
    for teacher in (True, False):
        w = (1.0, 0.0, 0.5)
        t = truth(lex, None, tea if teacher else None, 51, weights=w)
        _check(_run(lex, None, tea if teacher else None, 51, weights=w), t, f"no semantic scores teacher={teacher}")


@pytest.mark.gpu
def test_large_scores_padded_teacher_and_equal_rows():
    """scores of scale 200 and a teacher padded with -20 (ColBERT's layout): no NaN, within the bound; scores of magnitude 1e4; all-equal
    rows: the softmax is uniform up to the bound"""
    R, n = 6, 4
    Cn = R * n
    rng = np.random.default_rng(5)
    lex, sem = (_cast64(rng.normal(0, 200.0, (R, Cn)), "float32") for _ in range(2))
    tea = np.full((R, Cn), -20.0)
    for r in range(R):
        tea[r, r * n:(r + 1) * n] = _cast64(rng.normal(0, 5.0, n), "float32")
    for teacher in (tea, None):
        _check(_run(lex, sem, teacher, n), truth(lex, sem, teacher, n), f"scale 200 teacher={teacher is not None}")
    big = _cast64(rng.normal(0, 1e4, (R, Cn)), "float32")
    _check(_run(big, sem, tea, n), truth(big, sem, tea, n), "scale 1e4")
    flat = np.full((3, 257), 1.25)
    t = truth(flat, flat, flat, None)
    got = _run(flat, flat, flat, None)
    _check(got, t, "all-equal rows")
    assert abs(t["loss"]) < 1e-12 and np.abs(t["g_lex"]).max() < 1e-12
    t = truth(flat, flat, None, 2)
    got = _run(flat, flat, None, 2)
    _check(got, t, "all-equal rows, hard labels")
    off = np.ones((3, 257), bool)
    off[np.arange(3), np.arange(3) * 2] = False
    assert np.ptp(got[2][off]) <= 2 * t["b_lex"].max()          # uniform softmax: one value off the labels


@pytest.mark.gpu
def test_recipe_sized_step_with_cross_device_negatives():
    """(192, 1536, 8): 24 queries x 8 passages per device gathered from 8 ranks, --tct, and the hard-label form"""
    R, Cn, n = 192, 1536, 8
    lex, sem, tea = _seeded(R, Cn, 7, scale=4.0)
    _check(_run(lex, sem, tea, n), truth(lex, sem, tea, n), "recipe tct")
    _check(_run(lex, sem, None, n, weights=HARD_W), truth(lex, sem, None, n, weights=HARD_W), "recipe hard labels")


@pytest.mark.gpu
def test_wrappers_match_hybrid_loss():
    """dhr_loss, aggretriever_loss, contrastive_loss and distill_loss are the documented settings of hybrid_loss, bit for bit"""
    import torch
    from dhr_amd import train_loss as TL
    lex, sem, tea = (_dev(a, "float32") for a in _seeded(6, 24, 9))
    same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b))   # noqa: E731
    H = TL.hybrid_loss
    assert same(TL.dhr_loss(lex, sem, tea, train_n_passages=4, lamb=0.5, temperature=2.0), H(lex, sem, tea, train_n_passages=4, lamb=0.5, temperature=2.0))
    assert same(TL.dhr_loss(lex, sem, train_n_passages=4, lamb=1.0), H(lex, sem, train_n_passages=4, weights=HARD_W))
    assert same(TL.aggretriever_loss(lex, sem, tea, train_n_passages=4), H(lex, sem, tea, train_n_passages=4))
    assert same(TL.aggretriever_loss(lex, sem, train_n_passages=4), H(lex, sem, train_n_passages=4, weights=DHR_W))
    assert same(TL.aggretriever_loss(lex, train_n_passages=4), H(lex, train_n_passages=4, weights=HARD_W))
    assert torch.equal(TL.contrastive_loss(lex, 4), H(lex, train_n_passages=4, weights=HARD_W)[0])
    assert torch.equal(TL.distill_loss(lex, tea, 2.0), H(lex, None, tea, train_n_passages=1, temperature=2.0, weights=HARD_W, teacher_split=(1.0,) * 3)[0])
    want = torch.nn.functional.cross_entropy(lex.double(), torch.arange(6, device="cuda") * 4)
    assert abs(TL.contrastive_loss(lex, 4).item() - want.item()) < 1e-5 * abs(want.item())
    # empty batches: loss 0 as the entry point defines it
    loss, scores = H(lex[:0], sem[:0], train_n_passages=4)
    assert loss.item() == 0.0 and tuple(scores.shape) == (0, 24)


class _Spy:
    """the loaded library with every dhr_* call recorded"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("dhr_"):
            return fn

        def recorded(*args):
            self.calls.append((name, args))
            return fn(*args)
        return recorded


@pytest.mark.gpu
def test_bit_identity_upstream_scale_and_no_grad(monkeypatch):
    """Two runs: the same bits.  (loss * 8).backward(): 8 x the unit gradients, exactly (a power of two).  torch.no_grad(): the same loss
    bits, null gradient pointers at the library and no [R, C] gradient allocated.  One launch of the entry point per forward, none in the
    backward."""
    import torch
    from dhr_amd import train_loss as TL
    for (R, Cn, n), dtype in (((24, 192, 8), "float32"), ((5, 1025, 3), "float16")):
        lex, sem, tea = _seeded(R, Cn, 11, dtypes=(dtype,) * 3)
        for teacher in (tea, None):
            runs = []
            for scale in (1.0, 1.0, 8.0):
                tl, ts, tt = _dev(lex, dtype, True), _dev(sem, dtype, True), _dev(teacher, dtype)
                spy = _Spy(_lib.load())
                monkeypatch.setattr(_lib, "load", lambda: spy)
                loss, scores = TL.dhr_loss(tl, ts, tt, train_n_passages=n, lamb=1.0)
                (loss * scale).backward()
                monkeypatch.undo()
                assert [c[0] for c in spy.calls] == ["dhr_train_loss_workspace", "dhr_train_loss"]
                a = spy.calls[1][1]
                # grad_lexical and grad_semantic are filled by the forward
                assert a[21] not in (None, 0) and a[23] not in (None, 0) and a[-1] == torch.cuda.current_stream().cuda_stream
                runs.append((loss.detach(), scores, tl.grad, ts.grad))
            assert all(torch.equal(x, y) for x, y in zip(runs[0], runs[1]))
            assert torch.equal(runs[2][0], runs[0][0]) and torch.equal(runs[2][2], runs[0][2] * 8) and torch.equal(runs[2][3], runs[0][3] * 8)
            spy = _Spy(_lib.load())
            monkeypatch.setattr(_lib, "load", lambda: spy)
            with torch.no_grad():
                loss0, scores0 = TL.dhr_loss(tl, ts, tt, train_n_passages=n, lamb=1.0)
            loss1, _ = TL.dhr_loss(tl.detach(), ts.detach(), tt, train_n_passages=n, lamb=1.0)
            monkeypatch.undo()
            assert torch.equal(loss0, runs[0][0]) and torch.equal(loss1, runs[0][0]) and torch.equal(scores0, runs[0][1]) and not loss0.requires_grad
            assert [c[0] for c in spy.calls] == ["dhr_train_loss_workspace", "dhr_train_loss"] * 2
            assert all(c[1][21] is None and c[1][23] is None for c in spy.calls if c[0] == "dhr_train_loss")


@pytest.mark.gpu
def test_host_arrays_are_staged_and_match_the_device_path():
    """the entry point on host pointers (staged through the device, complete on return) gives the bits of the device path"""
    import torch
    from dhr_amd import train_loss as TL
    lib = _lib.load()
    R, Cn, n = 5, 255, 51
    lex, sem, tea = (a.astype(np.float32) for a in _seeded(R, Cn, 13))
    for teacher in (tea, None):
        loss, scores, gl, gs = (np.zeros(s, np.float32) for s in ((1,), (R, Cn), (R, Cn), (R, Cn)))
        p = lambda a: None if a is None else a.ctypes.data   # noqa: E731
        rc = lib.dhr_train_loss(0, _lib.MEM_HOST, p(lex), _lib.VAL_F32, Cn, p(sem), _lib.VAL_F32, Cn, p(teacher), _lib.VAL_F32, Cn, R, Cn, n, 1.0, 1.0,
                                (C.c_float * 3)(*DHR_W), (C.c_float * 3)(*SPLIT), p(loss), p(scores), Cn, p(gl), Cn, p(gs), Cn, None, 0, None)
        assert rc == _lib.DHR_OK, lib.dhr_last_error()
        tl, ts = _dev(lex, "float32", True), _dev(sem, "float32", True)
        d_loss, d_scores = TL.hybrid_loss(tl, ts, _dev(teacher, "float32"), train_n_passages=n)
        d_loss.backward()
        assert np.array_equal(loss, d_loss.detach().cpu().numpy().reshape(1)) and np.array_equal(scores, d_scores.cpu().numpy())
        assert np.array_equal(gl, tl.grad.cpu().numpy()) and np.array_equal(gs, ts.grad.cpu().numpy())
        assert isinstance(torch.cuda.current_stream().cuda_stream, int)


def _block(nbytes):
    """what torch's caching allocator charges for a tensor of nbytes: blocks of 512 bytes"""
    return -(-nbytes // 512) * 512


@pytest.mark.gpu
def test_memory_is_the_gradients_and_the_workspace():
    """(24, 192) fp32 with a teacher, forward + backward: the peak beyond what was allocated before the call and beyond the returned tensors
    (loss, scores, the two .grad) is at most the two saved gradients plus dhr_train_loss_workspace(R), each in the allocator's 512-byte
    blocks: no [R, C] temporary is allocated."""
    import torch
    from dhr_amd import train_loss as TL
    R, Cn, n = 24, 192, 8
    lex, sem, tea = _seeded(R, Cn, 17)
    tl, ts, tt = _dev(lex, "float32", True), _dev(sem, "float32", True), _dev(tea, "float32")
    TL.dhr_loss(tl, ts, tt, train_n_passages=n, lamb=1.0)[0].backward()          # warm-up: the library is loaded, kernels are resident
    tl.grad = ts.grad = None
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss, scores = TL.dhr_loss(tl, ts, tt, train_n_passages=n, lamb=1.0)
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    returned = sum(_block(t.numel() * t.element_size()) for t in (loss, scores, tl.grad, ts.grad))
    ws = int(_lib.load().dhr_train_loss_workspace(R))
    assert ws == R * 4
    extra, limit = peak - before - returned, 2 * _block(R * Cn * 4) + _block(ws)
    print(f"memory: peak {peak - before} B over the call, returned tensors {returned} B, the op's own {extra} B; limit {limit} B")
    assert extra <= limit


@pytest.mark.gpu
def test_stream_order(monkeypatch):
    """In the manner of tests/test_stream_order.py, whose harness this uses (read, not edited; its `check` knows only that file's entry
    points, so the assertions are restated here).  On a side stream behind a long-running blocker the call, forward and backward, returns
    before the blocker ends; after a stream synchronise the results are those of the default-stream run, bit for bit, although the buffers
    held other valid inputs (poison) when the call was made; dhr_train_loss received the side stream.  Then, with the blocker on the null
    stream instead, a call on the side stream completes while the blocker still runs: it does not wait on the null stream."""
    import torch
    from tests import test_stream_order as SO
    from dhr_amd import train_loss as TL
    blocker = SO._Blocker()
    R, Cn, n = 24, 192, 8

    def make(seed):
        g = SO._gen(seed)
        return dict(lex=SO._randn(g, (R, Cn), "float32", 3.0, True), sem=SO._randn(g, (R, Cn), "float16", 3.0, True), tea=SO._randn(g, (R, Cn), "float32", 3.0))

    def call(d):
        d["lex"].grad = d["sem"].grad = None
        loss, scores = TL.dhr_loss(d["lex"], d["sem"], d["tea"], train_n_passages=n, lamb=1.0)
        loss.backward()
        return loss.detach(), scores, d["lex"].grad, d["sem"].grad

    res = SO.run(make, call, blocker, monkeypatch, True)
    for k, r in enumerate(res.rounds):
        print(f"train_loss stream order round {k + 1}: blocker {r.block_ms:.1f} ms (needed {r.need_ms:.1f}), warmed host call {r.host_ms:.3f} ms, "
              f"returned early: {r.returned_early}, beside the null stream afterwards: {r.beside}, library calls: {[c[0] for c in r.calls]}")
        assert r.stream not in (None, 0) and len(r.got) == len(res.ref) == 4
        for i, (got, want) in enumerate(zip(r.got, res.ref)):
            assert got.shape == want.shape and got.dtype == want.dtype
            assert np.array_equal(SO._bits(got), SO._bits(want)), f"result {i} differs from the default-stream run: the op did not run in stream order"
        assert any(not np.array_equal(SO._bits(g), SO._bits(w)) for g, w in zip(r.on_poison, res.ref))
        assert [c[0] for c in r.calls] == ["dhr_train_loss_workspace", "dhr_train_loss"]
        assert r.calls[1][1][-1] == r.stream
    last = res.rounds[-1]
    assert last.need_ms <= SO.MAX_BLOCK_MS and last.block_ms >= last.need_ms and last.beside
    assert last.returned_early, f"in {len(res.rounds)} rounds the call returned only after its stream had caught up"

    # the null stream is busy: the call on a side stream neither runs on it nor waits for it
    s, _ = SO._side_stream(blocker)
    with torch.cuda.stream(s):
        d = SO._upload(make(1))
        call(d)
        s.synchronize()
    ref = tuple(t.clone() for t in res.ref)
    torch.cuda.synchronize()
    behind_null = torch.cuda.Event()
    with torch.cuda.stream(torch.cuda.default_stream()):
        blocker.enqueue(300.0)
        behind_null.record()
    with torch.cuda.stream(s):
        got = call(d)
        s.synchronize()
    still_running = not behind_null.query()
    torch.cuda.synchronize()
    assert still_running, "the call on a side stream completed only after the work on the null stream"
    assert all(np.array_equal(SO._bits(g), SO._bits(w)) for g, w in zip(got, ref))


def _eager(lex, sem, tea, lamb=1.0, temperature=1.0):
    """the reference's op sequence (DHR/modeling.py:170-187)"""
    import torch
    from torch import nn
    kl, softmax = nn.KLDivLoss(reduction="batchmean"), nn.Softmax(dim=-1)
    scores = lex + lamb * sem
    loss = 0
    loss += kl(nn.functional.log_softmax(scores, dim=-1), softmax(tea * temperature))
    loss += 0.5 * kl(nn.functional.log_softmax(sem, dim=-1), softmax(tea * temperature * 3 / 4))
    loss += 0.5 * kl(nn.functional.log_softmax(lex, dim=-1), softmax(tea * temperature * 1 / 4))
    return loss, scores


@pytest.mark.gpu
def test_timing_against_the_eager_composition():
    """Forward + backward at (24, 192) and (192, 1536), fp32, with a teacher: this library against the eager composition of the reference's
    ops, alternating in one process, device events around windows of 50 steps after 3 warm-up steps, three repeats.  One assertion: at
    (192, 1536) the fused step is faster than eager in every repeat -- the direction only, eager is some forty dependent launches and the
    fused step two.  The (24, 192) figures are printed."""
    import torch
    from dhr_amd import train_loss as TL
    for R, Cn, n in ((24, 192, 8), (192, 1536, 8)):
        lex, sem, tea = (_dev(a, "float32", g) for a, g in zip(_seeded(R, Cn, 19, scale=4.0), (True, True, False)))

        def fused():
            return TL.dhr_loss(lex, sem, tea, train_n_passages=n, lamb=1.0)

        def eager():
            return _eager(lex, sem, tea)

        def step(fn):
            lex.grad = sem.grad = None
            fn()[0].backward()

        def window(fn, steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                step(fn)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / steps

        times = {"fused": [], "eager": []}
        for _ in range(3):
            for name, fn in (("fused", fused), ("eager", eager)):
                window(fn, 3)
                times[name].append(window(fn, 50))
        f, e = times["fused"], times["eager"]
        step(fused)
        g_f = (lex.grad.clone(), sem.grad.clone())
        step(eager)
        assert all(torch.allclose(a, b, rtol=1e-3, atol=1e-7) for a, b in zip(g_f, (lex.grad, sem.grad)))      # the two sides time the same work
        print(f"train loss fwd+bwd R={R} C={Cn} fp32 tct: fused " + " / ".join(f"{t:.4f}" for t in f) + " ms, eager torch " +
              " / ".join(f"{t:.4f}" for t in e) + f" ms per step, {np.median(e) / np.median(f):.1f}x")
        if (R, Cn) == (192, 1536):
            assert all(a < b for a, b in zip(f, e)), (f, e)
