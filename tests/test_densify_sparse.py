"""Sparse densify (dhr_amd/densify_sparse.py, dhr_densify_sparse; densify/densify_corpus.py:29-93 and densify/densify_query.py of the reference).

CPU part (-m "not gpu"): the golden fixture (tests/golden/make_golden_densify_sparse.py: the reference's own outputs under NumPy >= 2) against
`fold`, a restatement of the reference's loop written here; the statuses of the entry point for every invalid argument; the wrappers' own
errors, raised before the library is touched; header, EXPORTS, build list and version script agree.
GPU part: the goldens bit for bit (values as uint16, indices, collisions); a seeded differential against `fold` over the row lengths, dims,
dtypes and id ranges at which the kernel takes another path; outputs inside wider arrays; host against device arrays; two runs; the command
lines in fresh child processes; stream order.  Nothing here reads the reference tree, and no test asserts a time."""
import fnmatch
import functools
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "densify_sparse_golden.npz")
LIMIT = {"int8": 127, "uint8": 255, "int16": 32767}


# ------------------------------------------------------------------------------------------ the restatement
def fold(ids, weights, omission, dims, vocab=None):
    """The reference's loop over one vector -> (float16 bits [dims] uint16, index [dims] int64, collisions).  `weights` is rounded to float16
    once, from the dtype it comes in; the comparison is between float16 values (a float16 is exact as a Python float)."""
    with np.errstate(over="ignore"):
        r16 = np.asarray(weights).astype(np.float16)
    bits, r = r16.view(np.uint16).tolist(), r16.astype(np.float64).tolist()
    value, vbits, index, collisions = [0.0] * dims, [0] * dims, [0] * dims, 0
    for n, t in enumerate(np.asarray(ids).tolist()):
        if t < omission or (vocab is not None and t >= vocab):
            continue
        s, g = (t - omission) % dims, (t - omission) // dims
        if value[s] == 0:
            value[s], vbits[s], index[s] = r[n], bits[n], g
        else:
            collisions += 1
            if value[s] < r[n]:
                value[s], vbits[s], index[s] = r[n], bits[n], g
    return np.array(vbits, np.uint16), np.array(index, np.int64), collisions


def fold_rows(indptr, ids, weights, omission, dims, vocab=None):
    nnz = len(ids)
    rows = []
    for b in range(len(indptr) - 1):
        lo, hi = (min(max(int(x), 0), nnz) for x in (indptr[b], indptr[b + 1]))
        rows.append(fold(ids[lo:hi], weights[lo:hi], omission, dims, vocab))           # (hi < lo: an empty slice)
    return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.array([r[2] for r in rows], np.int32))


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def golden_case(g, c):
    lo, hi, o0, o1 = int(g["case_ptr"][c]), int(g["case_ptr"][c + 1]), int(g["out_ptr"][c]), int(g["out_ptr"][c + 1])
    return g["ids"][lo:hi], g["weights"][lo:hi], g["value_bits"][o0:o1], g["index"][o0:o1]


# ------------------------------------------------------------------------------------------ CPU
def test_fixture_matches_the_restatement():
    g = golden()
    assert int(str(g["numpy_version"]).split(".")[0]) >= 2
    n = len(g["name"])
    assert n >= 100 and {int(x) for x in g["omission"]} == {472, 502, 570} and {int(x) for x in g["dims"]} == {8, 768} and {int(x) for x in g["wwm"]} == {0, 1}
    seen_collision = seen_negative = seen_inf = 0
    for c in range(n):
        ids, w, vbits, index = golden_case(g, c)
        got_bits, got_index, got_coll = fold(ids, w, int(g["omission"][c]), int(g["dims"][c]))
        name = str(g["name"][c])
        assert np.array_equal(got_bits, vbits), name
        assert np.array_equal(got_index, index.astype(np.int64)), name
        assert got_coll == int(g["collisions"][c]), name
        seen_collision += got_coll > 0
        seen_negative += bool(np.any(vbits > 0x8000))
        seen_inf += bool(np.any(vbits == 0x7C00))
    assert seen_collision and seen_negative and seen_inf
    # the edge behaviour of the contract, read off the reference's outputs: a zero-rounded entry sets the index and leaves the slice empty ...
    c = list(g["name"]).index("bm25-d8-negative-then-zero")
    _, _, vbits, index = golden_case(g, c)
    assert vbits[0] == 0xC200 and index[0] == 2            # -2, then 0 (replaces: -2 < 0), then -3 into the slice that is "empty" again
    assert vbits[1] == 0 and index[1] == 1 and int(g["collisions"][c]) == 1      # -0.0 then +0.0: no collision, the later group stays
    # ... and of two weights that tie only after the rounding the first keeps the slice
    for tag in ("near-one", "near-2048"):
        for rev in ("", "-reversed"):
            _, _, vbits, index = golden_case(g, list(g["name"]).index(f"unicoil-d768-tie-{tag}{rev}"))
            assert vbits[0] == vbits[1] and index[0] == 0 and index[1] == 1


def test_fixture_corpus_matches_the_restatement():
    import json
    g = golden()
    vocab = {t: n for n, t in enumerate(bytes(g["corpus_vocab"]).decode().splitlines())}
    docs = [json.loads(line) for line in bytes(g["corpus_jsonl"]).decode().splitlines()]
    assert [d["id"] for d in docs] == list(g["corpus_docids"]) and len(docs) == 40
    for n, d in enumerate(docs):
        bits, index, _ = fold([vocab[t] for t in d["vector"]], list(d["vector"].values()), 472, 16)
        assert np.array_equal(bits, g["corpus_value_bits"][n]) and np.array_equal(index, g["corpus_index"][n])


def _args(**kw):
    """valid arguments of dhr_densify_sparse on host arrays, one replaced at a time -> (ctypes arguments, keepalive)"""
    from dhr_amd import _lib
    a = dict(device=0, mem_kind=_lib.MEM_HOST, row_ptr=np.array([0, 2, 3], np.int64), ids=np.array([600, 700, 800], np.int64), id_bytes=8,
             weights=np.array([1, 2, 3], np.float32), weight_dtype=_lib.VAL_F32, nnz=3, batch=2, vocab=30522, omission=570, dims=768,
             value=np.zeros((2, 768), np.float16), value_dtype=_lib.VAL_F16, ld_value=768, index=np.zeros((2, 768), np.int8), index_dtype=_lib.IDX_I8,
             ld_index=768, collisions=np.zeros(2, np.int32), stream=None)
    a.update(kw)
    ptr = lambda x: None if x is None else x.ctypes.data
    return (a["device"], a["mem_kind"], ptr(a["row_ptr"]), ptr(a["ids"]), a["id_bytes"], ptr(a["weights"]), a["weight_dtype"], a["nnz"], a["batch"],
            a["vocab"], a["omission"], a["dims"], ptr(a["value"]), a["value_dtype"], a["ld_value"], ptr(a["index"]), a["index_dtype"], a["ld_index"],
            ptr(a["collisions"]), a["stream"]), a


INVALID = [("null row_ptr", dict(row_ptr=None)), ("null ids", dict(ids=None)), ("null weights", dict(weights=None)), ("null value", dict(value=None)),
           ("null index", dict(index=None)), ("mem_kind", dict(mem_kind=2)), ("mem_kind negative", dict(mem_kind=-1)), ("id_bytes 2", dict(id_bytes=2)),
           ("id_bytes 0", dict(id_bytes=0)), ("bf16 weights", dict(weight_dtype=2)), ("bf16 values", dict(value_dtype=2)),
           ("weight dtype", dict(weight_dtype=7)), ("no index dtype", dict(index_dtype=0)), ("index dtype", dict(index_dtype=4)),
           ("negative nnz", dict(nnz=-1)), ("negative batch", dict(batch=-1)), ("vocab 0", dict(vocab=0)), ("negative omission", dict(omission=-1)),
           ("omission at vocab", dict(omission=30522)), ("dims 0", dict(dims=0)), ("negative dims", dict(dims=-768)), ("short value stride", dict(ld_value=767)),
           ("short index stride", dict(ld_index=767)), ("group beyond int8", dict(vocab=570 + 768 * 128 + 1)),
           ("group beyond uint8", dict(index_dtype=1, vocab=570 + 768 * 256 + 1)), ("group beyond int16", dict(index_dtype=3, vocab=570 + 768 * 32768 + 1))]


@pytest.mark.parametrize("what, change", INVALID, ids=[w.replace(" ", "-") for w, _ in INVALID])
def test_invalid_arguments_are_refused(what, change):
    from dhr_amd import _lib
    lib = _lib.load()
    args, keep = _args(**change)
    assert lib.dhr_densify_sparse(*args) == _lib.ERR_INVALID, what
    assert lib.dhr_last_error()
    if what.startswith("group beyond"):
        assert b"group" in lib.dhr_last_error()


def test_statuses_of_the_limits():
    from dhr_amd import _lib
    lib = _lib.load()
    assert lib.dhr_version() == 105
    # the largest group that still fits is not refused for its size: with batch == 0 the call answers DHR_OK without touching a device
    for idt, groups in ((_lib.IDX_I8, 128), (_lib.IDX_U8, 256), (_lib.IDX_I16, 32768)):
        args, keep = _args(index_dtype=idt, vocab=570 + 768 * groups, batch=0)
        assert lib.dhr_densify_sparse(*args) == _lib.DHR_OK
    args, keep = _args(batch=0, nnz=0, ids=None, weights=None, collisions=None)         # nothing to read: the entry arrays may be absent
    assert lib.dhr_densify_sparse(*args) == _lib.DHR_OK
    args, keep = _args(dims=8193, ld_value=8193, ld_index=8193, index_dtype=_lib.IDX_I16)
    assert lib.dhr_densify_sparse(*args) == _lib.ERR_UNSUPPORTED and b"8192" in lib.dhr_last_error()
    args, keep = _args(dims=8193, ld_value=8193, ld_index=8192, index_dtype=_lib.IDX_I16)      # an invalid argument is named before the limit
    assert lib.dhr_densify_sparse(*args) == _lib.ERR_INVALID


def test_wrapper_errors_come_before_the_library(monkeypatch):
    from dhr_amd import _lib
    from dhr_amd import densify_sparse as DS

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    ptr, ids, w = np.array([0, 2], np.int64), np.array([600, 700], np.int64), np.array([1.0, 2.0], np.float32)
    with pytest.raises(ValueError, match="1-D"):
        DS.densify_vectors(ptr.reshape(1, 2), ids, w)
    with pytest.raises(ValueError, match="same length"):
        DS.densify_vectors(ptr, ids, w[:1])
    with pytest.raises(ValueError, match="batch \\+ 1"):
        DS.densify_vectors(ptr[:0], ids, w)
    for dims in (0, -1, 8193):
        with pytest.raises(ValueError, match="dims"):
            DS.densify_vectors(ptr, ids, w, dims)
    with pytest.raises(ValueError, match="omission"):
        DS.densify_vectors(ptr, ids, w, 768, -1)
    with pytest.raises(TypeError, match="integer"):
        DS.densify_vectors(ptr, ids.astype(np.float32), w)
    with pytest.raises(OverflowError, match="int8"):                                    # the reference: OverflowError when it meets such a term
        DS.densify_vectors(ptr, np.array([600, 570 + 768 * 128], np.int64), w)
    with pytest.raises(OverflowError, match="int16"):
        DS.densify_vectors(ptr, np.array([600, 472 + 8 * 32768], np.int64), w, 8, 472, True)
    with pytest.raises(ValueError, match="output arrays"):
        DS.densify_vectors_into(ptr, ids, w, np.zeros((1, 767), np.float16), np.zeros((1, 768), np.int8))
    with pytest.raises(ValueError, match="output arrays"):
        DS.densify_vectors_into(ptr, ids, w, np.zeros((2, 768), np.float16), np.zeros((2, 768), np.int8))
    with pytest.raises(TypeError, match="index_out"):
        DS.densify_vectors_into(ptr, ids, w, np.zeros((1, 768), np.float16), np.zeros((1, 768), np.int32))
    with pytest.raises(TypeError, match="value_out"):
        DS.densify_vectors_into(ptr, ids, w, np.zeros((1, 768), np.float64), np.zeros((1, 768), np.int8))
    import types
    with pytest.raises(KeyError):                                                       # an unknown term, as in the reference
        DS.densify({"vector": {"known": 1.0, "unknown": 2.0}}, 768, False, {"known": 600}, types.SimpleNamespace(model="unicoil"))
    # an empty block needs no library at all
    v, i, c = DS.densify_vectors(np.zeros(1, np.int64), ids[:0], w[:0], 8, 570, True)
    assert v.shape == (0, 8) and v.dtype == np.float16 and i.dtype == np.int16 and c.shape == (0,) and c.dtype == np.int32


def test_float64_weights_are_rounded_once():
    """1 + 2^-11 + 2^-30 lies above the tie between 1 and 1 + 2^-10: one rounding gives 1 + 2^-10; through float32 (which drops the 2^-30) it
    sits on the tie and falls to 1.  The wrapper's host conversion is the single step."""
    from dhr_amd import densify_sparse as DS
    w = np.array([1 + 2.0 ** -11 + 2.0 ** -30], np.float64)
    assert DS._half_or_float(w).view(np.uint16)[0] == 0x3C01 and w.astype(np.float32).astype(np.float16).view(np.uint16)[0] == 0x3C00
    _, _, w16 = DS._csr([{"a": float(w[0]), "b": 3}], {"a": 600, "b": 601})
    assert w16.dtype == np.float16 and w16.view(np.uint16).tolist() == [0x3C01, 0x4200]
    assert DS._half_or_float(np.array([2, 3], np.int64)).dtype == np.float16


def test_header_exports_build_list_and_map_agree():
    from dhr_amd import _build, _lib
    name = "dhr_densify_sparse"
    hdr = open(os.path.join(ROOT, "include", "dhr_hip.h")).read()
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S | re.M)
    assert m
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert len(params) == 20 and params[-1] == "void* stream" and params[2] == "const int64_t* row_ptr"
    assert name in _lib.EXPORTS and len(_lib.load().dhr_densify_sparse.argtypes) == len(params)
    assert "densify_sparse.hip" in _build.SOURCES
    src = open(os.path.join(ROOT, "dhr_amd", "csrc", "densify_sparse.hip")).read()
    assert re.search(r'^extern "C" int ' + name + r"\(", src, re.M) and "dhr::alloc_checkpoint()" in src and "DHR_CATCH_STATUS" in src
    vmap = open(os.path.join(ROOT, "dhr_amd", "csrc", "libdhr.map")).read()
    globs = re.findall(r"^\s*([a-z_*]+);", vmap.split("local:")[0], re.M)
    assert any(fnmatch.fnmatch(name, p) for p in globs), globs
    for f in ("__init__.py", "densify_corpus.py", "densify_query.py"):                 # the reference's module paths
        assert os.path.exists(os.path.join(ROOT, "densify", f))


# ------------------------------------------------------------------------------------------ GPU
def _bits(value):
    v = value if isinstance(value, np.ndarray) else value.cpu().numpy()
    return v.view(np.uint16)


def _np(t):
    return t if isinstance(t, np.ndarray) else t.cpu().numpy()


def _cuda(*arrays):
    import torch
    return tuple(torch.from_numpy(np.array(a)).cuda() for a in arrays)


@pytest.mark.gpu
def test_goldens_bit_for_bit():
    """every case of the fixture; the cases of one (omission, dims, index dtype) go through the library as one block, on host arrays and on
    device tensors, and the first block also vector by vector through the reference's `densify` signature"""
    import types
    from dhr_amd import densify_sparse as DS
    g = golden()
    keys = sorted({(int(g["omission"][c]), int(g["dims"][c]), int(g["wwm"][c])) for c in range(len(g["name"]))})
    assert len(keys) == 6                                  # (uniCOIL and SPLADE share omission and index dtype)
    for om, dims, wwm in keys:
        cs = [c for c in range(len(g["name"])) if (int(g["omission"][c]), int(g["dims"][c]), int(g["wwm"][c])) == (om, dims, wwm)]
        parts = [golden_case(g, c) for c in cs]
        indptr = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.int64)
        ids, w = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        want_bits, want_index = np.stack([p[2] for p in parts]), np.stack([p[3] for p in parts])
        want_coll = g["collisions"][cs]
        value, index, coll = DS.densify_vectors(indptr, ids, w, dims, om, bool(wwm))                 # float64 weights, host arrays
        assert value.dtype == np.float16 and index.dtype == (np.int16 if wwm else np.int8) and coll.dtype == np.int32
        assert np.array_equal(_bits(value), want_bits) and np.array_equal(index, want_index) and np.array_equal(coll, want_coll), (om, dims, wwm)
        with np.errstate(over="ignore"):
            tv, ti, tc = DS.densify_vectors(*_cuda(indptr, ids, w.astype(np.float16)), dims, om, bool(wwm))
        assert np.array_equal(_bits(tv), want_bits) and np.array_equal(_np(ti), want_index) and np.array_equal(_np(tc), want_coll), (om, dims, wwm)
    model = {472: "bm25", 502: "deepimpact", 570: "unicoil"}
    for c in range(len(g["name"])):
        if int(g["dims"][c]) != 8 or int(g["omission"][c]) != 472:
            continue
        ids, w, vbits, index = golden_case(g, c)
        weights = [int(x) for x in w] if int(g["is_int"][c]) else [float(x) for x in w]
        data = {"vector": {"t%d" % n: x for n, x in enumerate(weights)}}
        value, idx, coll = DS.densify(data, 8, True, {"t%d" % n: int(t) for n, t in enumerate(ids)}, types.SimpleNamespace(model=model[472]))
        assert value.shape == (8,) and np.array_equal(_bits(value), vbits) and np.array_equal(idx, index) and coll == int(g["collisions"][c]) and isinstance(coll, int)


ROWS = (0, 1, 63, 64, 65, 129, 70000)          # the 64-entry batches of a wave, and a row past any 16-bit position
# dims, index dtype, id dtype, weight dtype, signed: every dims at which the workgroup shape changes (4 rows per workgroup up to 4096, 2 at 8192),
# one that is no multiple of 64, one slice only; the three index dtypes; both id and weight dtypes
RANDOM = [(1, "int16", "int64", "float32", True), (8, "int8", "int32", "float16", False), (768, "int16", "int64", "float32", False),
          (768, "int8", "int32", "float32", True), (1000, "uint8", "int64", "float16", True), (4097, "int16", "int64", "float32", True),
          (8192, "int16", "int32", "float32", False), (8192, "uint8", "int64", "float16", True)]


def _weights(rng, n, signed, dtype):
    """A grid that forces ties after the rounding: 1 + j * 2^-12 (four neighbours share a float16, some of them through a round-to-even tie)
    at three scales; signed=True adds both zeros, negatives, weights that round to zero and to a float16 subnormal, and inf."""
    w = (1.0 + rng.integers(0, 16, n) * 2.0 ** -12) * rng.choice([1.0, 2048.0, 2.0 ** -10], n)
    if signed:
        kind = rng.integers(0, 8, n)
        w = np.where(kind == 0, -w, w)
        for k, x in ((1, 0.0), (2, -0.0), (3, 1e-9), (4, 4e-8), (5, -4e-8)):
            w = np.where(kind == k, x, w)
        w = np.where(rng.random(n) < 0.002, 70000.0, w)
    with np.errstate(over="ignore"):
        return w.astype(dtype)


@functools.lru_cache(maxsize=None)
def _random_case(dims, idt, id_dtype, w_dtype, signed):
    rng = np.random.default_rng(dims * 7 + len(idt) + signed)
    om = 472
    vocab = om + min(dims * (LIMIT[idt] + 1), 1_500_000) - 3                           # the last group is not whole
    lens = list(ROWS) + [int(x) for x in rng.integers(0, 200, 5)]
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(indptr[-1])
    ids = rng.integers(om, vocab, n)
    where = rng.random(n)
    ids = np.where(where < 0.05, rng.integers(0, om, n), ids)                          # omitted
    ids = np.where((where >= 0.05) & (where < 0.08), vocab + rng.integers(0, 5000, n), ids)      # beyond the vocabulary
    ids = np.where((where >= 0.08) & (where < 0.10), -1 - rng.integers(0, 5000, n), ids)         # negative
    hot = rng.random(n) < 0.3                                                          # repeated slices inside a 64-entry batch, also when dims is large
    ids = np.where(hot & (ids >= om) & (ids < vocab), om + ((ids - om) // dims) * dims + (ids - om) % min(dims, 5), ids)
    ids = ids.astype(id_dtype)
    w = _weights(rng, n, signed, w_dtype)
    for a in (indptr, ids, w):
        a.setflags(write=False)
    return indptr, ids, w, om, vocab, fold_rows(indptr, ids, w, om, dims, vocab)


@pytest.mark.gpu
@pytest.mark.parametrize("dims, idt, id_dtype, w_dtype, signed", RANDOM, ids=["-".join(str(x) for x in r) for r in RANDOM])
def test_random_differential(dims, idt, id_dtype, w_dtype, signed):
    import torch
    from dhr_amd import densify_sparse as DS
    indptr, ids, w, om, vocab, (want_bits, want_index, want_coll) = _random_case(dims, idt, id_dtype, w_dtype, signed)
    assert int(want_coll[6]) > 70000 * 0.8 - dims                                       # the long row collides almost everywhere
    t_ptr, t_ids, t_w = _cuda(indptr, ids, w)
    batch = len(indptr) - 1
    value = torch.full((batch, dims + 9), 7.0, dtype=torch.float16, device="cuda")
    index = torch.full((batch, dims + 3), 99, dtype=getattr(torch, idt), device="cuda")
    _, _, coll = DS.densify_vectors_into(t_ptr, t_ids, t_w, value, index, dims, om, vocab)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(value[:, :dims].contiguous()), want_bits)
    assert np.array_equal(_np(index[:, :dims]).astype(np.int64), want_index)
    assert np.array_equal(_np(coll), want_coll)
    assert bool((value[:, dims:] == 7.0).all()) and bool((index[:, dims:] == 99).all()), "sentinels beyond the record were overwritten"
    # a second run, into arrays with other row strides (even ones; odd above): the same bits, and the sentinels of these arrays intact too
    value2 = torch.full((batch, dims + 10), -3.0, dtype=torch.float16, device="cuda")
    index2 = torch.full((batch, dims + 4), 5, dtype=getattr(torch, idt), device="cuda")
    _, _, coll2 = DS.densify_vectors_into(t_ptr, t_ids, t_w, value2, index2, dims, om, vocab)
    assert torch.equal(value2[:, :dims].view(torch.int16), value[:, :dims].view(torch.int16)) and torch.equal(index2[:, :dims], index[:, :dims]) and torch.equal(coll, coll2)
    assert bool((value2[:, dims:] == -3.0).all()) and bool((index2[:, dims:] == 5).all()), "sentinels beyond the record were overwritten"
    # ... and a third run like the first: bit-identical
    value3, index3 = torch.full_like(value, 1.0), torch.full_like(index, 1)
    _, _, coll3 = DS.densify_vectors_into(t_ptr, t_ids, t_w, value3, index3, dims, om, vocab)
    assert torch.equal(value3[:, :dims].view(torch.int16), value[:, :dims].view(torch.int16))
    assert torch.equal(index3[:, :dims], index[:, :dims]) and torch.equal(coll3, coll)


@pytest.mark.gpu
def test_host_arrays_float32_values_and_strides():
    """host arrays against device arrays; float32 record values holding the float16-rounded weight; a row range that runs backwards, one
    beyond nnz and a negative one (empty / clamped); no collisions array through the C ABI"""
    import torch
    from dhr_amd import _lib
    from dhr_amd import densify_sparse as DS
    indptr, ids, w, om, vocab, (want_bits, want_index, want_coll) = _random_case(768, "int16", "int64", "float32", False)
    batch, dims = len(indptr) - 1, 768
    value = np.full((batch, dims + 5), 7.0, np.float32)
    index = np.full((batch, dims + 2), 99, np.int16)
    _, _, coll = DS.densify_vectors_into(indptr, ids, w, value, index, dims, om, vocab)
    assert np.array_equal(value[:, :dims].astype(np.float16).view(np.uint16), want_bits) and np.array_equal(value[:, :dims], want_bits.view(np.float16).astype(np.float32))
    assert np.array_equal(index[:, :dims], want_index) and np.array_equal(coll, want_coll)
    assert np.all(value[:, dims:] == 7.0) and np.all(index[:, dims:] == 99)
    # ranges: [5, 2) runs backwards, [2, nnz + 50) is cut at nnz, [-7, 3) starts at 0
    small_ids, small_w = ids[:200].copy(), w[:200].copy()
    ptr = np.array([5, 2, 250, -7, 3], np.int64)
    want = fold_rows(ptr, small_ids, small_w, om, dims, vocab)
    assert not want[0][0].any() and want[0][1].any() and want[0][3].any()          # the backward range is empty, the clamped ones are not
    lib = _lib.load()
    v, i = np.empty((4, dims), np.float16), np.empty((4, dims), np.int16)
    _lib.check(lib.dhr_densify_sparse(0, _lib.MEM_HOST, ptr.ctypes.data, small_ids.ctypes.data, 8, small_w.ctypes.data, _lib.VAL_F32, 200, 4, vocab, om,
                                      dims, v.ctypes.data, _lib.VAL_F16, dims, i.ctypes.data, _lib.IDX_I16, dims, None, None), "dhr_densify_sparse")
    assert np.array_equal(v.view(np.uint16), want[0]) and np.array_equal(i, want[1])


@pytest.mark.gpu
def test_batch_of_300():
    import torch
    from dhr_amd import densify_sparse as DS
    rng = np.random.default_rng(300)
    lens = rng.integers(0, 130, 300)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n, om, dims = int(indptr[-1]), 570, 768
    ids = rng.integers(0, 30522, n).astype(np.int32)
    w = _weights(rng, n, False, "float32")
    want_bits, want_index, want_coll = fold_rows(indptr, ids, w, om, dims)
    value, index, coll = DS.densify_vectors(*_cuda(indptr, ids, w), dims, om, False)
    assert value.dtype == torch.float16 and index.dtype == torch.int8 and coll.dtype == torch.int32 and value.is_cuda
    assert np.array_equal(_bits(value), want_bits) and np.array_equal(_np(index), want_index) and np.array_equal(_np(coll), want_coll)
    hv, hi, hc = DS.densify_vectors(indptr, ids, w, dims, om, False)
    assert np.array_equal(_bits(hv), want_bits) and np.array_equal(hi, want_index) and np.array_equal(hc, want_coll)


def _child(module, *args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", module] + list(args), cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)


@pytest.mark.gpu
def test_corpus_command_line(tmp_path):
    g = golden()
    vec_dir, out_dir = tmp_path / "vectors", tmp_path / "out"
    vec_dir.mkdir()
    (vec_dir / "docs.json").write_bytes(bytes(g["corpus_jsonl"]))
    (tmp_path / "vocab.txt").write_bytes(bytes(g["corpus_vocab"]))
    r = _child("densify.densify_corpus", "--model", "bm25", "--vocab_file", str(tmp_path / "vocab.txt"), "--vector_dir", str(vec_dir),
               "--output_dir", str(out_dir), "--output_dims", "16", "--prefix", "corpus")
    assert r.returncode == 0, r.stderr[-2000:]
    with open(out_dir / "encoding" / "corpus.split0.pt", "rb") as f:
        value, index, docids = pickle.load(f)
    assert value.dtype == np.float16 and index.dtype == np.int16 and value.shape == (40, 16)
    assert np.array_equal(value.view(np.uint16), g["corpus_value_bits"]) and np.array_equal(index, g["corpus_index"]) and docids == list(g["corpus_docids"])
    m = re.search(r"Total (\d+) collisions with 40 passages", r.stdout)
    assert m and int(m.group(1)) == 177                    # the total the reference printed for this corpus


@pytest.mark.gpu
def test_query_command_line(tmp_path):
    g = golden()
    vocab = bytes(g["corpus_vocab"]).decode().splitlines()
    (tmp_path / "vocab.txt").write_bytes(bytes(g["corpus_vocab"]))
    queries = [("q1", [vocab[500], vocab[516], vocab[500], vocab[10]]), ("q2", [vocab[480]] * 3 + [vocab[1271]])]
    (tmp_path / "dev.tsv").write_text("".join("%s\t%s\n" % (q, " ".join(t)) for q, t in queries))
    r = _child("densify.densify_query", "--model", "bm25", "--vocab_file", str(tmp_path / "vocab.txt"), "--query_path", str(tmp_path / "dev.tsv"),
               "--output_dir", str(tmp_path / "out"), "--output_dims", "16", "--prefix", "topics")
    assert r.returncode == 0, r.stderr[-2000:]
    with open(tmp_path / "out" / "encoding" / "queries" / "topics.dev.pt", "rb") as f:
        value, index, qids = pickle.load(f)
    assert qids == ["q1", "q2"] and value.dtype == np.float16 and index.dtype == np.int16
    # term frequencies as weights, first-seen order: q1 = {500: 2, 516: 1, 10: 1 (omitted)}; 500 and 516 share slice (500 - 472) % 16 = 12
    b0, i0, c0 = fold([500, 516, 10], [2, 1, 1], 472, 16)
    b1, i1, c1 = fold([480, 1271], [3, 1], 472, 16)
    assert np.array_equal(value.view(np.uint16), np.stack([b0, b1])) and np.array_equal(index, np.stack([i0, i1])) and c0 == 1
    assert "Total %d collisions with 2 queries" % (c0 + c1) in r.stdout


@pytest.mark.gpu
def test_stream_order(monkeypatch):
    """With the harness of tests/test_stream_order.py (`run` and its blocker; its `check` knows only that file's entry points, so what it
    asserts is restated here): behind a long blocker on a side stream the call returns early; its result equals the default-stream run bit
    for bit although the buffers held other valid vectors (poison) when it was made; on the poison it gives something else; and
    dhr_densify_sparse, the only library call, received torch's current stream as its last argument."""
    import torch
    from tests import test_stream_order as SO
    from dhr_amd import densify_sparse as DS
    blocker = SO._Blocker()
    lens = np.random.default_rng(5).integers(0, 90, 64)
    indptr = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
    n = int(indptr[-1])

    def make(seed):
        g = SO._gen(seed)
        return dict(ptr=indptr.clone(), ids=torch.randint(400, 30522, (n,), generator=g), w=torch.rand((n,), generator=g) * 9 + 0.05,
                    out_value=SO._full((64, 768 + 9), 7.0, "float16"), out_index=SO._full((64, 768 + 3), 99, "int8"))

    def call(d):
        _, _, coll = DS.densify_vectors_into(d["ptr"], d["ids"], d["w"], d["out_value"], d["out_index"], 768, 570)
        return d["out_value"], d["out_index"], coll

    res = SO.run(make, call, blocker, monkeypatch, True)
    for k, r in enumerate(res.rounds):
        print(f"densify_sparse stream order round {k + 1}: blocker {r.block_ms:.1f} ms (needed {r.need_ms:.1f}), warmed host call {r.host_ms:.3f} ms, "
              f"returned early: {r.returned_early}, beside the null stream afterwards: {r.beside}, library calls: {[c[0] for c in r.calls]}")
        assert r.stream not in (None, 0) and len(r.got) == len(res.ref) == 3
        for i, (got, want) in enumerate(zip(r.got, res.ref)):
            assert got.shape == want.shape and got.dtype == want.dtype
            assert np.array_equal(SO._bits(got), SO._bits(want)), f"result {i} differs from the default-stream run: the op did not run in stream order"
        assert any(not np.array_equal(SO._bits(g), SO._bits(w)) for g, w in zip(r.on_poison, res.ref))
        assert [c[0] for c in r.calls] == ["dhr_densify_sparse"]
        assert r.calls[0][1][-1] is not None and r.calls[0][1][-1] == r.stream
    last = res.rounds[-1]
    assert last.need_ms <= SO.MAX_BLOCK_MS and last.block_ms >= last.need_ms and last.beside
    assert last.returned_early, f"in {len(res.rounds)} rounds the call returned only after its stream had caught up"
