"""Streamed exact inner-product search over fp32 vectors (dhr_amd/stream_search.py on dhr_stream_search_*, csrc/stream_search.hip).

Truth is the float64 restatement below: s64(q, r) = <q, p_r> over both column segments, the k best rows by (score descending, row ascending),
(-inf, -1) beyond the rows seen.

The bound b(q, r) is derived from the arithmetic that was built, not measured.  Write A = sum_c |q_c p_c| over both segments, u = 2^-24.

 1. The split.  A row x is scaled by a power of two 2^e (exact) so that its largest magnitude lies in [2^14, 2^15); write v = x 2^e.
    hi = fp16(v), lo' = fp16((v - hi) 2^11), and the kernel uses v ~ hi + 2^-11 lo'.  fp16 has 11 significant bits, so |v - hi| <= 2^-11 |v| and
    v - hi is exact in fp32.  Where hi is normal ("N"), rounding lo' leaves at most 2^-11 |v - hi| <= 2^-22 |v|, or, where lo' is subnormal,
    at most 2^-25 2^-11 = 2^-36 absolutely.  Where fp16(v) would be subnormal ("F", |v| < 2^-14, that is |x| < 2^-28 max|x| of the row), hi = 0
    and lo' = fp16(v 2^11) carries the whole value with a relative error of 2^-11: at most 2^-25 absolutely in units of v.
 2. The products.  Of (hq + lq + eq)(hp + lp + ep) the kernel adds hq hp, hq lp and lq hp; lq lp and every product with an e are left out.
    Both N: |lq lp| <= 2^-22 |q p| (1 + 2^-10), the two e terms 2^-22 |q p| each: 3 * 2^-22 = 12 u, with the second order 12.5 u A.
    One F, say q: hq = 0, what is lost is lq lp + eq (hp + lp) <= (2^-11 + 2^-11)(1 + 2^-10) |q p| with |q| < 2^-28 max|q|: at most
    2^-38 (1 + 2^-9) max|q| |p_c|; the accumulation error of such full-size terms in the cross accumulator (item 3) adds 2^-15 of that.
    Both F: the product is lost whole, |q p| < 2^-56 max|q| max|p|.  The absolute errors of subnormal lo', divided by the other row's scale
    (>= 2^14 / max), are at most 2^-50 |q_c| max|p| and the like.  All absolute terms together stay below
        abs(q, r) = 2^-37 (max|q| sum_c |p_c| + max|p| sum_c |q_c|) + D 2^-56 max|q| max|p| ,     D = d_a + d_b .
    This is not below the 2^-40 sum|q_c| max|p| the issue hoped for: a flushed value keeps 11 bits, and it can be as large as 2^-28 of its
    row's maximum.  On case R it is 10^-5 of the relative part (printed).
 3. The accumulators.  Every product of two fp16 numbers is exact in fp32.  Per block of 128 columns the 128 products hq hp are added into one
    fp32 MFMA accumulator that starts at 0, the 256 cross products into a second one.  Each addition is charged 2^-23 of the partial sum's
    magnitude (2 u: round to nearest or truncation, in whatever order the MFMA adds its 16 products): 128 * 2 u = 256 u per block of
    sum |hq hp| <= (1 + 2^-10) |q p|, and 256 * 2 u * 2^-10 = 0.5 u for the cross products, which are 2^-11 of that each, two per column.
 4. The fold.  sum += (double) acc_hh + 2^-11 (double) acc_cross per block: two float64 roundings per block, 2 (D / 128) 2^-53 A < 2^-40 A.
 5. The sum is multiplied by 2^-(eq + ep) in float64 (exact) and rounded to fp32 once: u |s| <= u A.
    Hence  b(q, r) = 272 u A + abs(q, r)   (12.5 + 256.25 + 0.5 + 1 + what is left for the second orders), and b <= 2^-15 A = 512 u A is asserted.

On the grid cases every value is a multiple of 1/64 below 2^2 with at most 8 significant bits: hi is exact, lo' is 0, every product is a multiple
of 2^-12, A <= 13, so every partial sum is exact in fp32 and the answer must be the float64 answer bit for bit, ties included.

Case R (the softmax leak plus 20-80 real terms per passage): every returned score within b of the float64 score of its row; every returned row's
float64 score at least the float64 k-th score - 2 * 2^-15 max_r A; a query whose float64 gap between ranks k and k + 1 exceeds that band must
return exactly the float64 set; at most 3 of the 70 queries may fall under that exemption, asserted from the float64 values alone.

CPU part (-m "not gpu"): the symbols, the statuses that are decided before a device is touched, the wrapper's own errors.  GPU part: the rest."""
import ctypes as C
import fnmatch
import functools
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from dhr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
NEW = ("dhr_stream_search_create", "dhr_stream_search_add", "dhr_stream_search_result", "dhr_stream_search_device_bytes", "dhr_stream_search_destroy")
V, DS = 30522, 128


# ------------------------------------------------------------------------------------------ inputs and the float64 restatement
def make(seed, n, V, ds, lo, hi, grid):
    """the inputs of the issue, drawn in its order -> lex fp32 [n, V], sem fp32 [n, ds]"""
    rng = np.random.Generator(np.random.PCG64(seed))
    if grid:
        lex = np.zeros((n, V), np.float32)
        m = rng.random((n, V)) < 0.02
        lex[m] = rng.integers(1, 4, m.sum()) / 64
    else:
        lex = np.exp(rng.normal(-14.0, 2.0, (n, V))).astype(np.float32)            # the softmax leak
    p = 1 / np.arange(1, V + 1) ** 1.1
    p /= p.sum()
    perm = rng.permutation(V)
    for i in range(n):
        L = rng.integers(lo, hi + 1)
        cols = perm[rng.choice(V, L, replace=False, p=p)]
        lex[i, cols] = rng.integers(4, 129, L) / 64 if grid else rng.uniform(0.05, 2.0, L)
    sem = rng.integers(-32, 33, (n, ds)) / 64 if grid else rng.normal(0, 1, (n, ds)) * 0.1
    return lex, sem.astype(np.float32)


def topk64(s64, k, rows=None):
    """the k best of every query by (score descending, row ascending) -> scores fp32 [Q, k], rows int64 [Q, k], padded with (-inf, -1)"""
    Q, N = s64.shape
    rows = np.arange(N, dtype=np.int64) if rows is None else rows
    out_s, out_r = np.full((Q, k), -np.inf, np.float32), np.full((Q, k), -1, np.int64)
    for q in range(Q):
        o = np.lexsort((rows, -s64[q]))[:k]
        out_s[q, :len(o)], out_r[q, :len(o)] = s64[q, o].astype(np.float32), rows[o]
    return out_s, out_r


@functools.lru_cache(maxsize=None)
def case(name):
    """G1 / G2 / G3 / R of the issue -> the inputs, the float64 scores and what the checks need of them; computed once and left unchanged"""
    Q, N, d_a, d_b, k, grid = {"G1": (70, 600, V, DS, 100, True), "G2": (5, 300, 257, 0, 400, True), "G3": (40, 3000, 2051, 0, 50, True),
                               "R": (70, 600, V, DS, 20, False)}[name]
    qa, qb = make(3 if grid else 1, Q, d_a, d_b, 4, 12, grid)
    pa, pb = make(4 if grid else 2, N, d_a, d_b, 20, 80, grid)
    if name == "G1":
        pa[300], pb[300] = pa[3], pb[3]
    q64, p64 = np.concatenate([qa, qb], 1).astype(np.float64), np.concatenate([pa, pb], 1).astype(np.float64)
    s64 = q64 @ p64.T
    A = np.abs(q64) @ np.abs(p64).T
    k_s, k_r = topk64(s64, k)
    c = SimpleNamespace(name=name, Q=Q, N=N, d_a=d_a, d_b=d_b, k=k, qa=qa, qb=qb if d_b else None, pa=pa, pb=pb if d_b else None, s64=s64, A=A, top_s=k_s,
                        top_r=k_r, q64=q64, p64=p64)
    for a in (qa, qb, pa, pb, s64, A, k_s, k_r, q64, p64):
        a.setflags(write=False)
    return c


def bound(c):
    """b(q, r) of the module docstring -> (b, its absolute part)"""
    aq, ap = np.abs(c.q64), np.abs(c.p64)
    absolute = 2.0 ** -37 * (aq.max(1)[:, None] * ap.sum(1)[None, :] + ap.max(1)[None, :] * aq.sum(1)[:, None]) \
        + (c.d_a + c.d_b) * 2.0 ** -56 * aq.max(1)[:, None] * ap.max(1)[None, :]
    return 272 * U * c.A + absolute, absolute


# ------------------------------------------------------------------------------------------ CPU part
def test_new_symbols_are_declared_mapped_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "dhr_hip.h")).read()
    vmap = open(os.path.join(ROOT, "dhr_amd", "csrc", "libdhr.map")).read()
    globs = re.findall(r"^\s*([a-z_*]+);", vmap.split("local:")[0], re.M)
    lib = _lib.load()
    assert lib.dhr_version() == 105
    for name in NEW:
        assert name + "(" in header and name in _lib.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
        assert any(fnmatch.fnmatch(name, p) for p in globs), globs
        m = re.search(r"^(?:int|int64_t|void)\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S | re.M)
        assert m and len(m.group(1).split(",")) == len(getattr(lib, name).argtypes), name
        if "void* stream" in m.group(1):
            assert " ".join(m.group(1).split(",")[-1].split()) == "void* stream", name
    for name in NEW[:3]:
        assert re.search(r"^int\s+%s\s*\([^;]*void\* stream\)\s*;" % name, header, re.S | re.M), name
    assert lib.dhr_stream_search_device_bytes.restype is C.c_int64 and lib.dhr_stream_search_destroy.restype is None
    from dhr_amd import _build, beir_exact, stream_search
    assert "stream_search.hip" in _build.SOURCES
    for fn in ("add", "result", "device_bytes", "close"):
        assert callable(getattr(stream_search.StreamSearch, fn))
    assert callable(stream_search.search) and callable(beir_exact.ExactSearch.search)


def _bad_argument_calls(lib):
    """(what, call, status, text of dhr_last_error) for every bad argument that is refused before a device is touched"""
    q = np.zeros((4, 9), np.float32)
    qb = np.zeros((4, 3), np.float32)
    out = C.c_void_p()
    p = lambda a: a.ctypes.data                                # noqa: E731

    def create(kind=_lib.MEM_HOST, q_a=p(q), ld_qa=9, q_b=None, ld_qb=0, dtype=_lib.VAL_F32, n=4, d_a=9, d_b=0, k=3, block=0, res=C.byref(out)):
        return lib.dhr_stream_search_create(0, kind, q_a, ld_qa, q_b, ld_qb, dtype, n, d_a, d_b, k, block, res, None)

    def add(kind=_lib.MEM_HOST, p_a=p(q), dtype=_lib.VAL_F32, n=4, base=0):
        return lib.dhr_stream_search_add(None, kind, p_a, 9, None, 0, dtype, n, base, None)

    I, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    calls = [("create: null out", lambda: create(res=None), I, "null pointer"),
             ("create: null q_a", lambda: create(q_a=None), I, "null pointer"),
             ("create: mem_kind 7", lambda: create(kind=7), I, "bad mem_kind"),
             ("create: dtype 9", lambda: create(dtype=9), I, "bad value dtype"),
             ("create: fp16", lambda: create(dtype=_lib.VAL_F16), UNS, "must be fp32"),
             ("create: bf16", lambda: create(dtype=_lib.VAL_BF16), I, "bad value dtype"),
             ("create: d_a = 0", lambda: create(d_a=0), I, "d_a must be"),
             ("create: d_b < 0", lambda: create(d_b=-1), I, "d_a must be"),
             ("create: d_a + d_b too wide", lambda: create(d_a=131072, ld_qa=131072, d_b=1, q_b=p(qb), ld_qb=3), I, "d_a must be"),
             ("create: n_queries = 0", lambda: create(n=0), I, "n_queries must be"),
             ("create: n_queries = 65537", lambda: create(n=65537), I, "n_queries must be"),
             ("create: k = 0", lambda: create(k=0), I, "k must be"),
             ("create: k = 4097", lambda: create(k=4097), UNS, "k above 4096"),
             ("create: block_rows = 64", lambda: create(block=64), I, "block_rows must be"),
             ("create: block_rows = 200", lambda: create(block=200), I, "block_rows must be"),
             ("create: block_rows = 65664", lambda: create(block=65664), I, "block_rows must be"),
             ("create: q_b without d_b", lambda: create(q_b=p(qb), ld_qb=3), I, "q_b must be NULL exactly when d_b is 0"),
             ("create: d_b without q_b", lambda: create(d_b=3), I, "q_b must be NULL exactly when d_b is 0"),
             ("create: ld_qa < d_a", lambda: create(ld_qa=8), I, "row stride of q is shorter"),
             ("create: ld_qb < d_b", lambda: create(q_b=p(qb), d_b=3, ld_qb=2), I, "row stride of q is shorter"),
             ("add: mem_kind 7", lambda: add(kind=7), I, "bad mem_kind"),
             ("add: fp16", lambda: add(dtype=_lib.VAL_F16), UNS, "must be fp32"),
             ("add: n_rows < 0", lambda: add(n=-1), I, "n_rows must be"),
             ("add: row_base < 0", lambda: add(base=-1), I, "row_base must be"),
             ("add: null handle", lambda: add(), I, "null pointer"),
             ("result: null handle", lambda: lib.dhr_stream_search_result(None, p(q), p(q), _lib.MEM_HOST, None), I, "null pointer")]
    return calls, (q, qb, out)


def test_bad_arguments_are_refused_before_a_device_is_touched():
    lib = _lib.load()
    calls, keep = _bad_argument_calls(lib)
    for what, call, status, text in calls:
        assert call() == status, (what, lib.dhr_last_error())
        assert text in lib.dhr_last_error().decode(), (what, lib.dhr_last_error())
    assert keep[2].value is None                               # no handle came out of a refused create
    assert lib.dhr_stream_search_device_bytes(None) == 0
    lib.dhr_stream_search_destroy(None)


def test_wrapper_errors():
    from dhr_amd import stream_search as S
    q = np.zeros((4, 9), np.float32)
    with pytest.raises(ValueError, match="2-D"):
        S.StreamSearch(q[0])
    with pytest.raises(ValueError, match="k must be"):
        S.StreamSearch(q, k=4097)
    with pytest.raises(ValueError, match="k must be"):
        S.StreamSearch(q, k=0)
    with pytest.raises(ValueError, match="block_rows"):
        S.StreamSearch(q, k=3, block_rows=100)
    with pytest.raises(ValueError, match="rows"):
        S.StreamSearch(q, np.zeros((5, 3), np.float32))
    with pytest.raises(ValueError, match="columns"):
        S.StreamSearch(np.zeros((2, 131073), np.float32))


# ------------------------------------------------------------------------------------------ GPU part
def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the cases are read-only)


def _np(t):
    return t.detach().cpu().numpy() if not isinstance(t, np.ndarray) else t


def _bits(pair):
    s, r = _np(pair[0]), _np(pair[1])
    assert s.dtype == np.float32 and r.dtype == np.int64
    return s.view(np.uint32), r


def _same(got, want, what):
    (gs, gr), (ws, wr) = _bits(got), _bits(want)
    assert np.array_equal(gr, wr), f"{what}: {(gr != wr).sum()} rows differ, first at {np.argwhere(gr != wr)[:3].tolist()}"
    assert np.array_equal(gs, ws), f"{what}: {(gs != ws).sum()} scores differ in their bits"


def _run(c, qa, qb, chunks, k=None, block_rows=0):
    """chunks: (p_a, p_b, row_base or None)"""
    from dhr_amd.stream_search import StreamSearch
    with StreamSearch(qa, qb, k=k or c.k, block_rows=block_rows) as s:
        for pa, pb, base in chunks:
            s.add(pa, pb, row_base=base)
        assert s.device_bytes() > 0
        return s.result()


@functools.lru_cache(maxsize=None)
def g1_device():
    c = case("G1")
    return _dev(c.qa), _dev(c.qb), _dev(c.pa), _dev(c.pb)


@pytest.mark.gpu
def test_grid_g1_chunking_order_and_block_rows_give_the_float64_bits():
    c = case("G1")
    ties = [len(c.s64[q]) - len(np.unique(c.s64[q])) for q in range(c.Q)]
    print(f"G1: {min(ties)}-{max(ties)} exact ties per query; A <= {c.A.max():.2f}")
    assert c.A.max() <= 13 and min(ties) > 0
    qa, qb, pa, pb = g1_device()
    want = (c.top_s, c.top_r)
    _same(_run(c, qa, qb, [(pa, pb, None)]), want, "one add")
    cuts = [(0, 1), (1, 256), (256, 600)]
    _same(_run(c, qa, qb, [(pa[a:b], pb[a:b], None) for a, b in cuts]), want, "chunks of 1, 255 and 344 rows")
    _same(_run(c, qa, qb, [(pa[a:b], pb[a:b], a) for a, b in reversed(cuts)]), want, "the three chunks in reverse order")
    _same(_run(c, qa, qb, [(pa, pb, None)], block_rows=128), want, "block_rows = 128")
    r300 = (c.top_r == 300).any(1)
    assert r300.any() and all(list(c.top_r[q]).index(3) < list(c.top_r[q]).index(300) for q in np.flatnonzero(r300))         # the copy comes after row 3


@pytest.mark.gpu
def test_grid_g1_input_layouts():
    import torch
    c = case("G1")
    want = (c.top_s, c.top_r)
    got = _run(c, c.qa, c.qb, [(c.pa, c.pb, None)])
    assert isinstance(got[0], np.ndarray)
    _same(got, want, "host arrays")
    for extra, at_a, at_b, vec in ((5, 3, 3 + c.d_a + 1, 1), (6, 0, c.d_a + 2, 4)):      # rows aligned to nothing; rows aligned to 16 bytes
        width = c.d_a + c.d_b + extra
        views = []
        for a, b in ((c.qa, c.qb), (c.pa, c.pb)):
            wide = np.full((a.shape[0], width), 7.0, np.float32)
            wide[:, at_a:at_a + c.d_a], wide[:, at_b:at_b + c.d_b] = a, b
            t = _dev(wide)
            views += [t[:, at_a:at_a + c.d_a], t[:, at_b:at_b + c.d_b]]
        assert all(v.stride(0) == width and (v.data_ptr() % 16 == 0) == (vec == 4) for v in views)
        _same(_run(c, views[0], views[1], [(views[2], views[3], None)]), want, f"views into one [n, {width}] matrix")
    # one concatenated matrix as segment a alone; queries on the host against passages on the device
    qcat, pcat = np.concatenate([c.qa, c.qb], 1), _dev(np.concatenate([c.pa, c.pb], 1))
    got = _run(c, qcat, None, [(pcat, None, None)])
    assert isinstance(got[0], np.ndarray)
    _same(got, want, "one concatenated segment")
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_grid_g2_k_beyond_the_rows_and_an_empty_add():
    c = case("G2")
    assert c.k > c.N and (c.top_r[:, c.N:] == -1).all() and np.isneginf(c.top_s[:, c.N:]).all()
    qa, pa = _dev(c.qa), _dev(c.pa)
    from dhr_amd.stream_search import StreamSearch, search
    with StreamSearch(qa, None, k=c.k) as s:
        _same(s.result(), (np.full((c.Q, c.k), -np.inf, np.float32), np.full((c.Q, c.k), -1, np.int64)), "before any add")
        s.add(pa[:0])
        s.add(pa[:131]).add(pa[131:])
        first = s.result()
        _same(first, (c.top_s, c.top_r), "G2")
        _same(s.result(), first, "a second result")
        assert s.rows_added == c.N
    _same(search(c.qa, [c.pa[:7], c.pa[7:]], k=c.k), (c.top_s, c.top_r), "search() over host chunks")


@pytest.mark.gpu
def test_grid_g3_threshold_worst_and_best_feed_order():
    c = case("G3")
    qa = _dev(c.qa)
    up = np.argsort(c.s64[0], kind="stable")
    answers = []
    for what, order in (("ascending", up), ("descending", up[::-1].copy())):
        s64 = c.s64[:, order]                                 # the scores in the numbering of this feed
        got = _run(c, qa, None, [(_dev(c.pa[order]), None, None)], block_rows=256)
        _same(got, topk64(s64, c.k), f"rows fed in {what} score of query 0")
        answers.append((_np(got[0]), order[_np(got[1])]))
    assert np.array_equal(answers[0][0].view(np.uint32), answers[1][0].view(np.uint32))
    for q in range(c.Q):                                      # above the k-th score the two feeds hold the same rows of the corpus
        inner = answers[0][0][q] > answers[0][0][q, -1]
        assert set(answers[0][1][q, inner]) == set(answers[1][1][q, inner]), q


@pytest.mark.gpu
def test_a_nan_row_enters_no_list_and_changes_no_other_score():
    c = case("G1")
    qa, qb, pa, pb = g1_device()
    bad = pa.clone()
    bad[7, 100] = float("nan")
    got = _run(c, qa, qb, [(bad, pb, None)])
    assert not (_np(got[1]) == 7).any() and not np.isnan(_np(got[0])).any()
    s64 = c.s64.copy()
    s64[:, 7] = -np.inf
    want_s, want_r = topk64(s64, c.k)
    assert (c.top_r == 7).any() and not (want_r == 7).any()
    _same(got, (want_s, want_r), "G1 without row 7")


@pytest.mark.gpu
def test_side_stream_gives_the_default_stream_bits():
    import torch
    c = case("G3")
    base = _run(c, _dev(c.qa), None, [(_dev(c.pa), None, None)], block_rows=256)
    _same(base, (c.top_s, c.top_r), "G3 on the default stream")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        qa, pa = _dev(c.qa), _dev(c.pa)
        got = _run(c, qa, None, [(pa[:1000], None, None), (pa[1000:], None, None)], block_rows=256)
    side.synchronize()
    _same(got, base, "G3 on a side stream")


@pytest.mark.gpu
def test_bad_passages_are_refused_by_a_live_search():
    lib = _lib.load()
    c = case("G2")
    from dhr_amd.stream_search import StreamSearch
    with StreamSearch(c.qa, None, k=5) as s:
        pa = np.ascontiguousarray(c.pa[:4])
        sem = np.zeros((4, 3), np.float32)
        add = lambda p_a=pa.ctypes.data, ld=c.d_a, p_b=None, ld_b=0: lib.dhr_stream_search_add(s._h, _lib.MEM_HOST, p_a, ld, p_b, ld_b, _lib.VAL_F32, 4, 0, None)  # noqa: E731
        for what, call, text in (("null p_a", lambda: add(p_a=None), "null pointer"), ("ld < d_a", lambda: add(ld=c.d_a - 1), "row stride of p is shorter"),
                                 ("p_b without d_b", lambda: add(p_b=sem.ctypes.data, ld_b=3), "p_b must be NULL exactly when d_b is 0")):
            assert call() == _lib.ERR_INVALID, what
            assert text in lib.dhr_last_error().decode(), (what, lib.dhr_last_error())
        with pytest.raises(ValueError, match="columns"):
            s.add(np.zeros((4, c.d_a + 1), np.float32))
        _same(s.result(), (np.full((c.Q, 5), -np.inf, np.float32), np.full((c.Q, 5), -1, np.int64)), "after refused adds")


@pytest.mark.gpu
def test_realistic_case_against_float64_with_the_derived_bound():
    import torch
    c = case("R")
    b, absolute = bound(c)
    print(f"R: max b / (2^-15 A) = {(b / (2.0 ** -15 * c.A)).max():.4f}; largest absolute part / b = {(absolute / b).max():.2e}")
    assert (b <= 2.0 ** -15 * c.A).all()
    band = 2 * 2.0 ** -15 * c.A.max(1)                          # per query
    ranked = -np.sort(-c.s64, axis=1)
    gap = ranked[:, c.k - 1] - ranked[:, c.k]
    unclear = gap <= band
    print(f"R: {unclear.sum()} of {c.Q} queries have a float64 gap between ranks {c.k} and {c.k + 1} inside the band; median gap {np.median(gap / band):.1f} bands")
    assert unclear.sum() <= 3                                  # from the float64 values alone, before the device is asked
    got_s, got_r = (_np(x) for x in _run(c, _dev(c.qa), _dev(c.qb), [(_dev(c.pa[:333]), _dev(c.pb[:333]), None), (_dev(c.pa[333:]), _dev(c.pb[333:]), None)]))
    assert ((got_r >= 0) & (got_r < c.N)).all() and all(len(set(got_r[q])) == c.k for q in range(c.Q))
    qi = np.arange(c.Q)[:, None]
    err = np.abs(got_s.astype(np.float64) - c.s64[qi, got_r])
    mm = torch.mm(torch.from_numpy(np.concatenate([c.qa, c.qb], 1)), torch.from_numpy(np.concatenate([c.pa, c.pb], 1)).T).numpy().astype(np.float64)
    print(f"R: max |s - s64| / (2^-24 A) = {(err / (U * c.A[qi, got_r])).max():.3f} on the device, "
          f"{(np.abs(mm - c.s64) / (U * c.A)).max():.3f} for torch.mm in fp32 on the CPU; max |s - s64| / b = {(err / b[qi, got_r]).max():.4f}")
    assert (err <= b[qi, got_r]).all(), f"a score is {(err / b[qi, got_r]).max():.3f} b off the float64 score of its row"
    assert (np.diff(got_s, axis=1) <= 0).all()
    assert (c.s64[qi, got_r] >= ranked[:, c.k - 1][:, None] - band[:, None]).all()
    for q in np.flatnonzero(~unclear):
        assert set(got_r[q]) == set(c.top_r[q]), q
