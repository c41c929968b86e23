"""dhr_search_excluding / GipIndex.search(exclude=...): the exact search in which query q never returns a row of its exclusion list.

Checked as smoke() checks a search -- oracle.gip_oracle.gip_scores_f64 and check_topk -- on the score vector with the excluded rows taken
out and the returned row ids mapped to positions in what remains; DHR_PARAM_CAND_CAP 1024 so that the bound GEMM, refine and rescoring all
run.  Every query excludes its own unfiltered top-5, 20 random rows and one row outside the shard."""
import ctypes as C

import numpy as np
import pytest

from dhr_amd import _lib, synth
from oracle import gip_oracle as O

pytestmark = pytest.mark.gpu

K = 100
CORPORA = {"hybrid": (5, 3000, 8, 768, 128, "encoder"), "dense": (10, 3000, 8, 0, 768, "dense"), "bm25_int16": (11, 3000, 8, 768, 0, "bm25")}
_pairs = {}


def pair(name):
    """(corpus values, corpus index, fp32 queries, query index, float64 scores [Q, N]) of a corpus, computed once and left unchanged"""
    if name not in _pairs:
        seed, n, q, d_dlr, d_cls, kind = CORPORA[name]
        cv, ci, qv, qi = synth.make_pair(seed, n, q, d_dlr, d_cls, kind=kind)
        q32 = qv.astype(np.float32)
        c32 = cv.astype(np.float32)
        ex = np.stack([O.gip_scores_f64(q32[i], None if qi is None else qi[i], c32, ci) for i in range(q)])
        for a in (cv, ci, q32, qi, ex):
            if a is not None:
                a.setflags(write=False)
        _pairs[name] = (cv, ci, q32, qi, ex)
    return _pairs[name]


def open_index(name, row_offset=0):
    from dhr_amd.retrieval.gip_retrieval import GipIndex
    cv, ci, _, _, _ = pair(name)
    ix = GipIndex(cv, ci, device=0, row_offset=row_offset)
    ix.set_param(_lib.PARAM_CAND_CAP, 1024)
    return ix


def exclusions(rows_plain, n, row_offset, seed):
    """per query: its own unfiltered top-5, 20 random rows of the shard and one row outside it, global ids, shuffled"""
    rng = np.random.default_rng(seed)
    return [rng.permutation(np.concatenate([rows_plain[i, :5], row_offset + rng.choice(n, 20, replace=False),
                                            [row_offset + n + 17 + i]]).astype(np.int64)) for i in range(rows_plain.shape[0])]


def check_against_oracle(scores, rows, lists, ex, k, row_offset=0):
    n = ex.shape[1]
    for i in range(rows.shape[0]):
        banned = np.unique(lists[i]) - row_offset
        banned = banned[(banned >= 0) & (banned < n)]
        remain = np.setdiff1d(np.arange(n), banned)
        kk = min(k, len(remain))
        assert np.all(rows[i, :kk] >= 0), "fewer real entries than rows remain"
        assert np.all(rows[i, kk:] == -1) and np.all(np.isneginf(scores[i, kk:]))
        local = rows[i, :kk] - row_offset
        assert not np.isin(local, banned).any(), "an excluded row came back"
        pos = np.searchsorted(remain, local)
        assert np.array_equal(remain[pos], local)
        O.check_topk(pos, scores[i, :kk], ex[i][remain], kk)


@pytest.mark.parametrize("name", list(CORPORA))
def test_excluded_rows_never_return_and_the_rest_is_the_exact_topk(name):
    _, _, q32, qi, ex = pair(name)
    n = ex.shape[1]
    ix = open_index(name)
    s0, r0 = ix.search(q32, qi, K)
    lists = exclusions(r0, n, 0, 3)
    s1, r1 = ix.search(q32, qi, K, exclude=lists)
    st = ix.stats()
    s2, r2 = ix.search(q32, qi, K, exclude=_lib.make_exclusions(lists)[:2])          # the same lists as a CSR pair
    ix.close()
    assert st["k"] == K + 26 and st["phases"] >= 1, st            # the underlying search, at depth k + the longest list
    assert np.all(r1 >= 0)                                         # every list has k real entries
    check_against_oracle(s1, r1, lists, ex, K)
    for i in range(r0.shape[0]):                                   # the top-5 of the plain search are gone, what follows moved up
        assert not np.isin(r0[i, :5], r1[i]).any()
    np.testing.assert_array_equal(r2, r1)
    np.testing.assert_array_equal(s2.view(np.uint32), s1.view(np.uint32))


def test_empty_exclusions_are_the_plain_search_bit_for_bit():
    _, _, q32, qi, _ = pair("hybrid")
    ix = open_index("hybrid")
    s0, r0 = ix.search(q32, qi, K)
    for empty in ([[] for _ in range(q32.shape[0])], (np.zeros(q32.shape[0] + 1, np.int64), np.zeros(0, np.int64))):
        s1, r1 = ix.search(q32, qi, K, exclude=empty)
        assert ix.stats()["k"] == K
        assert np.array_equal(r1, r0) and np.array_equal(s1.view(np.uint32), s0.view(np.uint32))
    ix.close()


def test_row_offset_index_takes_global_rows():
    _, _, q32, qi, ex = pair("hybrid")
    off = 10_000
    ix = open_index("hybrid", row_offset=off)
    s0, r0 = ix.search(q32, qi, K)
    assert r0.min() >= off
    lists = exclusions(r0, ex.shape[1], off, 4)
    s1, r1 = ix.search(q32, qi, K, exclude=lists)
    # local ids in the list are other rows (or none) of a shard that starts at 10 000: nothing of the plain top-k may vanish for them
    s2, r2 = ix.search(q32, qi, K, exclude=[r0[i, :5] - off for i in range(r0.shape[0])])
    ix.close()
    check_against_oracle(s1, r1, lists, ex, K, row_offset=off)
    check_against_oracle(s2, r2, [r0[i, :5] - off for i in range(r0.shape[0])], ex, K, row_offset=off)


def test_k_equal_to_the_corpus_leaves_exactly_the_excluded_rows_as_padding():
    _, _, q32, qi, ex = pair("hybrid")
    n = ex.shape[1]
    ix = open_index("hybrid")
    rng = np.random.default_rng(8)
    lists = [rng.choice(n, 7, replace=False).astype(np.int64) for _ in range(q32.shape[0])]
    s1, r1 = ix.search(q32, qi, n, exclude=lists)
    ix.close()
    assert np.all(r1[:, : n - 7] >= 0) and np.all(r1[:, n - 7:] == -1) and np.all(np.isneginf(s1[:, n - 7:]))
    check_against_oracle(s1, r1, lists, ex, n)


def test_k_prime_beyond_the_limit_is_unsupported_and_names_both_numbers():
    _, _, q32, qi, _ = pair("hybrid")
    ix = open_index("hybrid")
    lists = [np.arange(77, dtype=np.int64)] + [[] for _ in range(q32.shape[0] - 1)]
    with pytest.raises(_lib.DhrError) as ei:
        ix.search(q32, qi, (1 << 20) - 50, exclude=lists)
    ix.close()
    assert ei.value.status == _lib.ERR_UNSUPPORTED and str((1 << 20) - 50) in str(ei.value) and "77" in str(ei.value)


def test_exclude_rows_filters_lists_from_elsewhere_in_both_memory_kinds():
    """GipIndex.exclude_rows on the lists of a deeper plain search = search(exclude=...), from numpy and from torch cuda arrays"""
    import torch
    _, _, q32, qi, ex = pair("hybrid")
    ix = open_index("hybrid")
    s0, r0 = ix.search(q32, qi, K + 26)
    lists = exclusions(r0, ex.shape[1], 0, 3)
    s1, r1 = ix.search(q32, qi, K, exclude=lists)
    hs, hr, hv = ix.exclude_rows(s0, r0, lists, K, return_valid=True)
    ds, dr = ix.exclude_rows(torch.from_numpy(s0).cuda(), torch.from_numpy(r0).cuda(), lists, K)
    ix.close()
    assert isinstance(hs, np.ndarray) and ds.is_cuda and dr.is_cuda and hv.tolist() == [K] * r0.shape[0]
    for gs, gr in ((hs, hr), (ds.cpu().numpy(), dr.cpu().numpy())):
        assert np.array_equal(gr, r1) and np.array_equal(gs.view(np.uint32), s1.view(np.uint32))


def test_out_device_on_a_side_stream_completes_in_stream_order(monkeypatch):
    """The poison-then-wait arrangement of tests/test_stream_order.py (its harness imported: `run`, the blocker, the side-stream probe): behind a
    blocker on a side stream the real queries and exclusion rows are copied over poison, then the search is called on that stream.  A search
    that ran on another stream, or read its inputs before the stream reached them, returns what the poison gives."""
    import torch
    from tests.test_stream_order import MAX_BLOCK_MS, _Blocker, _bits, run
    _, _, q32, qi, ex = pair("hybrid")
    Q, n = q32.shape[0], ex.shape[1]
    ix = open_index("hybrid")
    _, r_plain = ix.search(q32, qi, K)
    ptr = np.arange(Q + 1, dtype=np.int64) * 26

    def make_inputs(seed):          # seed 1: the real batch; seed 2: the same queries in another order with other lists
        roll = seed - 1
        lists = exclusions(np.roll(r_plain, roll, axis=0), n, 0, seed)
        return {"qv": torch.from_numpy(np.roll(q32, roll, axis=0).copy()), "qi": torch.from_numpy(np.roll(qi, roll, axis=0).copy()),
                "ex": torch.from_numpy(np.concatenate(lists))}

    def call(b):
        ix._lib = _lib.load()       # (the harness swaps the loader for a spy that records every call into the library)
        return ix.search(b["qv"], b["qi"], K, out_device=True, stream=torch.cuda.current_stream().cuda_stream, exclude=(ptr, b["ex"]))

    res = run(make_inputs, call, _Blocker(), monkeypatch, no_wait=False)
    ix._lib = _lib.load()
    want_s, want_r = ix.search(q32, qi, K, exclude=(ptr, make_inputs(1)["ex"].numpy()))      # host arrays, default stream
    ix.close()
    assert np.array_equal(res.ref[1].cpu().numpy(), want_r) and np.array_equal(_bits(res.ref[0]), want_s.view(np.uint8).reshape(-1))
    for r in res.rounds:
        assert r.stream not in (None, 0)
        for g, w in zip(r.got, res.ref):
            assert g.is_cuda and np.array_equal(_bits(g), _bits(w)), "the search did not run in stream order"
        assert any(not np.array_equal(_bits(g), _bits(w)) for g, w in zip(r.on_poison, res.ref))
        assert not r.returned_early                  # the call waits for its stream: the result is complete on return
        names = [c[0] for c in r.calls if c[0] != "dhr_last_error"]
        assert names == ["dhr_search_excluding"], names
        assert all(c[1][-1] == r.stream for c in r.calls if c[0] == "dhr_search_excluding")
    last = res.rounds[-1]
    assert last.need_ms <= MAX_BLOCK_MS and last.block_ms >= last.need_ms and last.beside, vars(last)


def test_every_host_allocation_failure_is_nomem_and_the_handle_works_again():
    """the sweep of tests/test_abi_guard.py (_sweep) through dhr_search_excluding on a warm handle, with dhr_debug_fail_alloc alone"""
    lib = _lib.load()
    _, _, q32, qi, ex = pair("hybrid")
    Q = q32.shape[0]
    ix = open_index("hybrid")
    ix.set_param(_lib.PARAM_PROFILE, 1)                  # (the timers allocate too)
    _, r_plain = ix.search(q32, qi, K)
    ptr, rows, _, _ = _lib.make_exclusions(exclusions(r_plain, ex.shape[1], 0, 3))
    qb, keep = _lib.make_query_batch(q32, qi)
    s0, r0, s1, r1 = np.zeros((Q, K), np.float32), np.zeros((Q, K), np.int64), np.zeros((Q, K), np.float32), np.zeros((Q, K), np.int64)

    def call(s, r):
        return lib.dhr_search_excluding(ix._h, C.byref(qb), K, ptr.ctypes.data, rows.ctypes.data, _lib.MEM_HOST, s.ctypes.data, r.ctypes.data,
                                        _lib.MEM_HOST, None)
    assert call(s0, r0) == 0                             # warm: the workspace and the staging buffer exist
    a0 = lib.dhr_debug_fail_alloc(0)
    assert call(s0, r0) == 0
    n_alloc = lib.dhr_debug_fail_alloc(0) - a0
    assert n_alloc >= 3
    for i in range(1, n_alloc + 1):
        lib.dhr_debug_fail_alloc(i)
        rc = call(s1, r1)
        lib.dhr_debug_fail_alloc(0)
        assert rc == _lib.ERR_NOMEM and b"memory" in lib.dhr_last_error(), (i, n_alloc, rc, lib.dhr_last_error())
        assert call(s1, r1) == 0                         # the handle is usable right away
        assert np.array_equal(r1, r0) and np.array_equal(s1.view(np.uint32), s0.view(np.uint32)), i
    ix.close()
    del keep
