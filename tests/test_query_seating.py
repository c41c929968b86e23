"""Seating of the queries for the main pass (DHR_PARAM_SEAT_QUERIES; dhr_amd/csrc/seating.h, search_core.hip, gemm_g8.hip): after the sampled run
of a whole search on the integer bound GEMM the batch is seated in the kernel's query tiles by descending length of its bound lists, so that
the few hot queries share wave columns.  Nothing a query computes depends on its slot: with the switch off and on a search returns the same
lists bit for bit, passes the same candidates through both filters and launches the same plan -- and both equal the float64 oracle.

Shape: 40 000 rows x (768 + 64), sample period 4 -- the smallest corpus of tests/golden/controller_plan.json's cases on which the sampled
controller runs (n40000_period4); the int8 image of the gated half puts it on gemm_filter_g8_kernel (checked: DHR_INFO_GEMM_KERNEL), the fp16
image on gemm_filter_wx_kernel, which never seats.  DHR_PARAM_LIST_STRIDE = 1 024 gives the hot queries a second list tier.

Planted queries (about 1 % of a batch):
  HOT    the 32 slices of the corpus's most frequent terms (a sliding window per query) at weight 30, with an index value no row has: no gated
         product counts in the exact score, so the k-th best score is a dense-only one, while in every slice the rows that share the value's
         bucket -- about half of them -- count their entry in the bound: nearly every row passes the bound filter.  (A query that carries the
         frequent terms WITH their index values is not hot: measured here at half the median list -- its exact scores are as large as its
         bounds.  A list is long where the bucketed bound is loose.)  Their lists must be at least 30 x the batch's median, asserted from the
         list lengths themselves;
  FLOOD  the same at weight 3 on 32 less frequent slices: more than EPI_STACK = 32 of the 64 rows a lane holds of it pass (asserted from
         the bound scores), so the surplus scan and the second list tier run under the map."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import gip_oracle as O

pytestmark = pytest.mark.gpu

N_ROWS, D_DLR, D_CLS, K, PERIOD = 40_000, 768, 64, 30, 4
NQ_MAX = 700
HOT = (5, 131, 260, 300, 417, 599, 650)      # HOT[:6] lie in a 600-query batch, all seven in a 700-query one
FLOOD = 77
EPI_STACK = 32                               # gemm_common.h


@functools.lru_cache(maxsize=1)
def _data():
    from dhr_amd import synth
    cv, ci, qv, qi = synth.make_pair(5150, N_ROWS, NQ_MAX, D_DLR, D_CLS)
    q32 = qv.astype(np.float32)
    qi = qi.copy()
    # the corpus's most frequent terms: (slice, index value) pairs of entries above the background, by row count, one per slice
    live = cv[:, :D_DLR].astype(np.float32) > synth.BG_MAX
    cnt = np.zeros((D_DLR, 256), np.int64)
    np.add.at(cnt, (np.nonzero(live)[1], ci[live].astype(np.int64)), 1)
    order = np.argsort(-cnt.max(1), kind="stable")           # slices by the row count of their most frequent term
    absent = 255
    assert not (ci == absent).any()
    for h, q in enumerate(HOT):
        sl = order[h:h + 32]                                 # a sliding window: every hot query is a different one
        q32[q, :D_DLR] = 0.0
        q32[q, sl] = 30.0
        qi[q, sl] = absent
    sl = order[100:132]
    q32[FLOOD, :D_DLR] = 0.0
    q32[FLOOD, sl] = 3.0
    qi[FLOOD, sl] = absent
    for a in (cv, ci, q32, qi):
        a.setflags(write=False)
    return cv, ci, q32, qi


_EXACT = {}


def _exact(i):
    """float64 oracle scores of query i against the corpus, computed once per session and shared."""
    if i not in _EXACT:
        cv, ci, q32, qi = _data()
        _EXACT[i] = O.gip_scores_f64(q32[i], qi[i], _c32(), ci)
        _EXACT[i].setflags(write=False)
    return _EXACT[i]


@functools.lru_cache(maxsize=1)
def _c32():
    return _data()[0].astype(np.float32)


def _check_oracle(scores, rows, queries):
    for i in queries:
        ex = _exact(i)
        O.check_topk(rows[i, :K], scores[i, :K], ex, K)
        np.testing.assert_allclose(scores[i, :K], ex[rows[i, :K]].astype(np.float32), rtol=0, atol=1e-6 * max(1.0, np.abs(ex).max()))


def _index(overlap):
    from dhr_amd import _lib
    from dhr_amd.retrieval.gip_retrieval import GipIndex
    cv, ci, _, _ = _data()
    ix = GipIndex(cv, ci)
    ix.set_param(_lib.PARAM_PROFILE, 1)
    ix.set_param(_lib.PARAM_SAMPLE_PERIOD, PERIOD)
    ix.set_param(_lib.PARAM_LIST_STRIDE, 1024)
    if not overlap:      # candidate counts then do not depend on how the two streams interleave (test_refine_two_level.py)
        ix.set_param(_lib.PARAM_OVERLAP_AUX, 0)
    return ix


def _seating(ix, nq):
    """dhr_debug_query_seating -> None (identity) or dict of the host arrays."""
    from dhr_amd import _lib
    n = (nq + 255) // 256 * 256
    out = {"slot_q": np.full(n, -1, np.int32), "q_slot": np.full(n, -1, np.int32), "len": np.zeros(n, np.uint32),
           "thr_seat": np.zeros(n, np.float32), "thr_hat": np.zeros(n, np.float32)}
    rc = ix._lib.dhr_debug_query_seating(ix._h, n, *[out[f].ctypes.data for f in ("slot_q", "q_slot", "len", "thr_seat", "thr_hat")])
    if rc < 0:
        _lib.check(rc, "dhr_debug_query_seating")
    return out if rc == 1 else None


PLAN_FIELDS = ("phases", "gemm_rows", "candidates_bound", "candidates_exact", "overflow_retries", "sample_fallback_queries")


@pytest.mark.parametrize("nq", [600, 700, 256])
def test_equal_results(nq, gated_image):
    """(a) 600 queries: three tiles, the last with 88 real queries (the partial path); (b) 700: the last tile holds 188 (the full path);
    (c) 256: one tile, identity seating."""
    from dhr_amd import _lib
    _, _, q32, qi = _data()
    q, qx = q32[:nq], qi[:nq]
    ix = _index(overlap=False)
    try:
        ix.set_param(_lib.PARAM_SEAT_QUERIES, 0)
        s0, r0 = ix.search(q, qx, K)
        st0 = ix.stats()
        assert _seating(ix, nq) is None
        ix.set_param(_lib.PARAM_SEAT_QUERIES, -1)
        s1, r1 = ix.search(q, qx, K)
        st1 = ix.stats()
        seat = _seating(ix, nq)
        kernel = int(ix.info(_lib.INFO_GEMM_KERNEL))
        print("query_seating nq %d %s: kernel %d, seated %s, %s" % (nq, gated_image, kernel, seat is not None, {f: (st0[f], st1[f]) for f in PLAN_FIELDS}))
        np.testing.assert_array_equal(r1, r0)
        np.testing.assert_array_equal(s1.view(np.uint32), s0.view(np.uint32))
        for f in PLAN_FIELDS:
            assert st1[f] == st0[f], (f, st0[f], st1[f])
        hot = [h for h in HOT if h < nq]
        _check_oracle(s1, r1, sorted(set(hot + [FLOOD, 0, 1, nq // 2, nq - 1])))
        if gated_image != "gated_i8":
            assert kernel in (3, 4) and seat is None          # the fp16-gated kernels never seat
            return
        assert kernel == 5
        if nq <= 256:
            assert seat is None                               # one query tile: nothing to seat, the second tile buffer is not written
            return
        assert seat is not None
        assert not np.array_equal(seat["slot_q"], np.arange(len(seat["slot_q"])))      # the seating really moved queries
        ln = seat["len"][:nq].astype(np.int64)
        med = float(np.median(ln))
        print("  bound-list lengths of the sampled run: median %.0f, hot %s, flood %d" % (med, ln[hot].tolist(), ln[FLOOD]))
        assert med > 0
        assert (ln[hot] >= 30 * med).all(), (ln[hot].tolist(), med)
        assert 0.005 * nq <= len(hot) + 1 <= 0.015 * nq
        # the flood query fills a lane's hit stack: more than EPI_STACK of the 64 rows one lane holds of it (rows of a 128-row half tile whose
        # bit 2 is the lane half) reach even the final threshold, which no threshold of the pass exceeded
        qb, keep = _lib.make_query_batch(q[FLOOD:FLOOD + 1], qx[FLOOD:FLOOD + 1])
        import torch
        U = torch.empty((1, 4096), dtype=torch.float32, device="cuda")
        _lib.check(ix._lib.dhr_debug_bound_scores(ix._h, C.byref(qb), 0, 4096, U.data_ptr(), None), "dhr_debug_bound_scores")
        hit = (U[0].cpu().numpy() >= seat["thr_hat"][FLOOD]).reshape(-1, 128)            # [half tile][row]
        per_lane = np.stack([hit[:, ((np.arange(128) >> 2) & 1) == h].sum(1) for h in (0, 1)])
        print("  flood query: at most %d of a lane's 64 rows pass the final threshold" % per_lane.max())
        assert per_lane.max() > EPI_STACK
    finally:
        ix.close()


def test_permutation(force_gated_i8):
    """slot_q and q_slot are inverse permutations of [0, Q_pad), real queries sit in front of padded ones, and the order is numpy.lexsort on
    (-length, query number) of the lengths the hook returns."""
    _, _, q32, qi = _data()
    nq = 600
    ix = _index(overlap=False)
    try:
        ix.search(q32[:nq], qi[:nq], K)
        seat = _seating(ix, nq)
    finally:
        ix.close()
    assert seat is not None
    q_pad = 768
    slot_q, q_slot = seat["slot_q"].astype(np.int64), seat["q_slot"].astype(np.int64)
    assert np.array_equal(np.sort(slot_q), np.arange(q_pad)) and np.array_equal(np.sort(q_slot), np.arange(q_pad))
    assert np.array_equal(slot_q[q_slot], np.arange(q_pad)) and np.array_equal(q_slot[slot_q], np.arange(q_pad))
    assert (slot_q[:nq] < nq).all() and np.array_equal(slot_q[nq:], np.arange(nq, q_pad))
    ln = seat["len"][:nq].astype(np.int64)
    assert np.array_equal(slot_q[:nq], np.lexsort((np.arange(nq), -ln)))
    assert (seat["len"][nq:] == 0).all()


def test_live_thresholds(force_gated_i8):
    """Default overlap: refine / rescoring / select raise the thresholds beside the next chunk's bound GEMM; every such write keeps the
    slot-ordered mirror current, so after the search it equals thr_hat[slot_q] bitwise.  (Candidate counts are not compared here: they depend
    on how the two streams interleave.)"""
    _, _, q32, qi = _data()
    nq = 700
    ix = _index(overlap=True)
    try:
        s, r = ix.search(q32[:nq], qi[:nq], K)
        seat = _seating(ix, nq)
    finally:
        ix.close()
    assert seat is not None
    np.testing.assert_array_equal(seat["thr_seat"].view(np.uint32), seat["thr_hat"][seat["slot_q"]].view(np.uint32))
    assert np.isposinf(seat["thr_seat"][nq:]).all() and np.isfinite(seat["thr_seat"][:nq]).all()
    _check_oracle(s, r, sorted(set(list(HOT) + [FLOOD, 0, 1, nq // 2, nq - 1])))


def test_identity_paths(force_gated_i8):
    """Staged (begin / finish) and sharded calls keep every query where the caller put it: the same index gives what it gives with the
    switch off, and the hook reports no seating."""
    import torch
    from dhr_amd import _lib, dist as D
    from dhr_amd.retrieval import gip_retrieval as G
    cv, ci, q32, qi = _data()
    nq = 600
    q, qx = q32[:nq], qi[:nq]

    def staged(ix):
        sample = ix.search_begin(q, qx, K)
        tau = sample.min(dim=1).values if sample is not None else None
        s, r, c = ix.search_finish(tau)
        assert _seating(ix, nq) is None
        return s.cpu().numpy(), r.cpu().numpy(), c.cpu().numpy()

    ix = _index(overlap=False)
    try:
        ix.set_param(_lib.PARAM_SEAT_QUERIES, 0)
        off = staged(ix)
        ix.set_param(_lib.PARAM_SEAT_QUERIES, -1)
        on = staged(ix)
    finally:
        ix.close()
    for a, b in zip(off, on):
        np.testing.assert_array_equal(a, b)

    shards = []
    try:
        for sh in range(2):
            lo, hi = G.shard_bounds(N_ROWS, 2, sh)
            shards.append(G.GipIndex(cv[lo:hi], ci[lo:hi], row_offset=lo))
            shards[-1].set_param(_lib.PARAM_SAMPLE_PERIOD, PERIOD)
            shards[-1].set_param(_lib.PARAM_SEAT_QUERIES, 0)
        s0, r0 = D.search_sharded_local(shards, q, qx, K)
        s0, r0 = s0.cpu().numpy(), r0.cpu().numpy()
        for sh in shards:
            sh.set_param(_lib.PARAM_SEAT_QUERIES, -1)
        s1, r1 = D.search_sharded_local(shards, q, qx, K)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(r1.cpu().numpy(), r0)
        np.testing.assert_array_equal(s1.cpu().numpy().view(np.uint32), s0.view(np.uint32))
    finally:
        for sh in shards:
            sh.close()
    _check_oracle(s0, r0, [HOT[0], FLOOD, 1, nq - 1])
