"""GPU parity tests: the HIP path (through the C ABI / ctypes) against the oracle and against the
golden vectors produced by the reference.  Run on the MI355X box with `pytest -m gpu`."""
import os
import tempfile
import zlib

import numpy as np
import pytest

from oracle import gip_oracle as O
from tests.util import case_args, dump_pickle, parse_trec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    from dhr_amd.retrieval import gip_retrieval as G_
    from dhr_amd import _lib
    _lib.load()
    return G_


def _search_check(G, cv, ci, qv32, qi, k, *, params=(), emb_dim=None, queries=None, row_offset=0, idx_buckets=0):
    from dhr_amd import _lib
    ix = G.GipIndex(cv, ci, row_offset=row_offset, idx_buckets=idx_buckets)
    for p, v in params:
        ix.set_param(p, v)
    ix.set_param(_lib.PARAM_PROFILE, 1)
    scores, rows = ix.search(qv32, qi, k)
    st = ix.stats()
    ix.close()
    n = cv.shape[0]
    c32 = cv.astype(np.float32)
    for i in (queries if queries is not None else range(qv32.shape[0])):
        ex = O.gip_scores_f64(qv32[i], None if qi is None else qi[i], c32, ci)
        kk = min(k, n)
        assert np.all(rows[i, kk:] == -1) and np.all(np.isneginf(scores[i, kk:]))
        O.check_topk(rows[i, :kk] - row_offset, scores[i, :kk], ex, k)
        # exactly rounded scores: fp32(round(exact f64))
        np.testing.assert_allclose(scores[i, :kk], ex[rows[i, :kk] - row_offset].astype(np.float32), rtol=0, atol=1e-6 * max(1.0, np.abs(ex).max()))
    return scores, rows, st


def _i8_margin(ix, qv32, d_cls):
    """Upper bound of the per-query bound of |<q,d> - mul <q8,d8>| over the ungated columns of a dense_i8 index (query_prep_kernel,
    kernels.hip): ||q'|| * max_r ||d' - sc d8|| + ||q' - sq q8|| * max_r ||sc d8||, where q' = q * w (column weights w <= 1) and
    every entry of q' - sq q8 is at most sq / 2 with sq <= max(max |q_dense| / 127, max |q_gated| / 60000)."""
    from dhr_amd import _lib
    ec, nc = ix.info(_lib.INFO_I8_ROW_ERR), ix.info(_lib.INFO_I8_ROW_NORM)
    qd = qv32[:, qv32.shape[1] - d_cls:].astype(np.float32)
    qg = np.abs(qv32[:, :qv32.shape[1] - d_cls]).max(axis=1, initial=0.0)
    am = np.abs(qd).max(axis=1)
    sq = np.maximum(np.where(am > 0, am / np.float32(127), np.float32(1)), qg / np.float32(60000)).astype(np.float32)
    return 1.01 * (np.linalg.norm(qd, axis=1) * ec + 0.5 * np.sqrt(d_cls) * sq * nc) + 1e-2


def test_bound_gemm_layout(G, golden):
    """The MFMA bound GEMM (stage images, swizzle, fragment mapping of the 2:4 and the dense matrix instructions): with ONE index bucket
    (idx_buckets = 1: every index value in bucket 0) the bound is the plain inner product Q x D^T of the non-negative operands; with the
    default two buckets it is still an upper bound of the gated score, and a tighter one; an ungated batch (--IP stage 1) gets the plain
    inner product again.  (More than two buckets went with the K-step tile layout in round 6: DHR_ERR_UNSUPPORTED.)"""
    import ctypes as C
    import torch
    from dhr_amd import _lib
    d = golden.inputs("hyb")
    cv = d["cv"][:1000]                      # ragged: not a multiple of 256
    qv = d["qv"].astype(np.float32)
    qb, keep = _lib.make_query_batch(qv, d["qi"])
    out = torch.zeros((qv.shape[0], 1000), dtype=torch.float32, device="cuda")
    ref = qv.astype(np.float64) @ cv.astype(np.float64).T
    exact = np.stack([O.gip_scores_f64(qv[i], d["qi"][i], cv.astype(np.float32), d["ci"][:1000]) for i in range(qv.shape[0])])
    slack = {}
    for nb in (1, 2):
        ix = G.GipIndex(cv, d["ci"][:1000], idx_buckets=nb)
        _lib.check(ix._lib.dhr_debug_bound_scores(ix._h, C.byref(qb), 0, 1000, out.data_ptr(), 0), "debug_bound")
        ub = out.cpu().numpy().astype(np.float64)
        # an int8 image of the ungated columns (DHR_INFO_DENSE_I8) is off by at most what the filter margin pays; its gated operands
        # are rounded UP in units of the int8 scale
        tol = 1e-3 + (_i8_margin(ix, qv, cv.shape[1] - d["ci"].shape[1]).max() if ix.info(_lib.INFO_DENSE_I8) else 0.0)
        # (a gated_i8 index rounds every gated operand UP by at most one int8 level: the bound may exceed the plain inner product)
        up = 0.05 * np.abs(ref).max() if ix.info(_lib.INFO_GATED_I8) else 2e-3 * np.abs(ref).max() if ix.info(_lib.INFO_DENSE_I8) else 0.0
        assert np.all(ub >= exact - tol) and np.all(ub <= ref + tol + up)
        if nb == 1:
            assert np.all(ub >= ref - tol)                 # one bucket: nothing is gated away
        slack[nb] = float((ub - exact).mean())
        if nb == 2:      # ungated query batch (--IP stage 1) on the bucketed index: the bound is the plain inner product again
            qb2, keep2 = _lib.make_query_batch(qv, None)
            _lib.check(ix._lib.dhr_debug_bound_scores(ix._h, C.byref(qb2), 0, 1000, out.data_ptr(), 0), "debug_bound")
            u2 = out.cpu().numpy().astype(np.float64)
            assert np.all(u2 >= ref - tol) and np.all(u2 <= ref + tol + up)
        ix.close()
    assert slack[2] < slack[1] and slack[1] <= float((ref - exact).mean()) + 0.06 * np.abs(ref).max()
    with pytest.raises(_lib.DhrError) as ei:
        G.GipIndex(cv, d["ci"][:1000], idx_buckets=3)
    assert ei.value.status == _lib.ERR_UNSUPPORTED


@pytest.mark.parametrize("kind", ["hybrid", "no_ungated", "ungated_batch", "abs_mode"])
def test_g8_bound_layout(G, kind, force_gated_i8):
    """The integer bound GEMM of a gated_i8 index (gemm_g8.hip: 2:4 int8 stage images, position words, fragment mapping, the shift
    between the two halves) == the restated integer bound (oracle/g8_bound_oracle.py), and >= the exact score - margin.  Corpus and
    query index values are drawn from two values per slice with equal mass, which the bucket maps separate: a bucket match is then
    an index match, and the restatement needs no map."""
    import ctypes as C
    import torch
    from dhr_amd import _lib, synth
    from oracle import g8_bound_oracle as G8
    rng = np.random.default_rng(zlib.crc32(kind.encode()))
    n, nq, d, c = 1000, 70, 128, 0 if kind == "no_ungated" else 192
    cg, _ = synth.make_dlr(rng, n, d, 10, 30)
    qg, _ = synth.make_dlr(rng, nq, d, 3, 8)
    cg, qg = cg.astype(np.float32), qg.astype(np.float32)
    if kind == "abs_mode":
        cg *= np.where(rng.random(cg.shape) < 0.3, -1, 1).astype(np.float32)
        qg *= np.where(rng.random(qg.shape) < 0.3, -1, 1).astype(np.float32)
    pair = rng.integers(0, 100, (d, 2)); pair[:, 1] = pair[:, 0] + 1 + rng.integers(0, 100, d)
    ci = np.take_along_axis(np.broadcast_to(pair[None], (n, d, 2)), rng.integers(0, 2, (n, d, 1)), axis=2)[..., 0].astype(np.uint8)
    qi = np.take_along_axis(np.broadcast_to(pair[None], (nq, d, 2)), rng.integers(0, 2, (nq, d, 1)), axis=2)[..., 0].astype(np.int16)
    cd = (rng.standard_normal((n, c)) * 0.1).astype(np.float32)
    qd = (rng.standard_normal((nq, c)) * 0.1).astype(np.float32)
    cv = np.concatenate([cg, cd], axis=1).astype(np.float16)
    qv = np.concatenate([qg, qd], axis=1).astype(np.float32)
    cv32 = cv.astype(np.float32)
    ix = G.GipIndex(cv, ci)
    assert ix.info(_lib.INFO_GATED_I8) == 1
    gated_batch = kind != "ungated_batch"
    qb, keep = _lib.make_query_batch(qv, qi if gated_batch else None)
    out = torch.zeros((nq, n), dtype=torch.float32, device="cuda")
    _lib.check(ix._lib.dhr_debug_bound_scores(ix._h, C.byref(qb), 0, n, out.data_ptr(), 0), "debug_bound")
    ub = out.cpu().numpy().astype(np.float64)
    ix.close()
    if gated_batch:
        U, margin = G8.bound_scores(qv[:, :d], qi, qv[:, d:], cv32[:, :d], ci, cv32[:, d:], abs_mode=kind == "abs_mode")
        exact = np.stack([O.gip_scores_f64(qv[i], qi[i], cv32, ci) for i in range(nq)])
    else:       # plain inner product over a gated index: every slice counts
        z = np.zeros_like(ci)
        U, margin = G8.bound_scores(qv[:, :d], z[:nq], qv[:, d:], cv32[:, :d], z, cv32[:, d:], abs_mode=kind == "abs_mode")
        exact = qv.astype(np.float64) @ cv32.astype(np.float64).T
        if kind == "abs_mode":
            exact = np.abs(qv[:, :d]).astype(np.float64) @ np.abs(cv32[:, :d]).astype(np.float64).T + qv[:, d:].astype(np.float64) @ cv32[:, d:].astype(np.float64).T
    assert np.all(ub >= exact - margin[:, None] - 1e-6), float((ub - exact + margin[:, None]).min())
    # the device's fp32 arithmetic carries ~1e-6 of head room, so single int8 levels may differ from the float64 restatement
    diff = np.abs(ub - U)
    scale = np.abs(U).max()
    assert np.quantile(diff, 0.99) <= 1e-4 * scale and diff.max() <= 0.02 * scale, (float(np.quantile(diff, 0.99)), float(diff.max()), float(scale))


@pytest.mark.parametrize("mode", ["gated_i8", "gated_fp16"])
@pytest.mark.parametrize("kind", ["bench", "adversarial"])
def test_bound_never_below_exact_minus_margin(G, monkeypatch, mode, kind):
    """The inequality the filter rests on, measured at the benchmark's width (768 gated + 768 ungated columns) over ALL pairs of
    64 queries x 1 M rows of the bench corpus, and over adversarial inputs: U[q][row] >= exact_f64[q][row] - margin[q].  A bound
    that fell short would silently drop a true top-k row; the minimum head room is printed.  Both images of the gated half: the
    int8 one (integer sums, every rounding up, margin = the ungated Cauchy-Schwarz term) and the fp16 one (fp32 accumulation on
    top of the 2^23 offset of the int8 stages)."""
    import ctypes as C
    import torch
    import bench
    from dhr_amd import _lib, synth
    monkeypatch.setenv("DHR_GATED_I8", "1" if mode == "gated_i8" else "0")
    dev = torch.device("cuda", 0)
    nq, d = 64, 768
    if kind == "bench":
        n = 1_000_000
        cv, ci = bench.gen_shard(torch, synth, dev, 1237, n, d, d, 30, 90, False)
        qv, qi = bench.gen_shard(torch, synth, dev, 1237 + 999_983, nq, d, d, 4, 12, False)
        qv = qv.float()
    else:
        n = 200_000
        cv, ci = bench.gen_shard(torch, synth, dev, 99, n, d, d, 30, 90, True)
        qv, qi = bench.gen_shard(torch, synth, dev, 98, nq, d, d, 4, 12, True)
        g = torch.Generator(device=dev).manual_seed(5)
        cv = cv.float(); qv = qv.float()
        cv[:4000, :d] = 3.0                                       # max-norm rows
        cv[:, d + 5] *= 50; cv[:, d + 70] *= 30; cv[:, 11] *= 20   # outlier columns, ungated and gated
        cv[4000:4400, :d] = torch.where(torch.rand((400, d), generator=g, device=dev) < 0.02, torch.full((400, d), 900.0, device=dev), cv[4000:4400, :d])   # huge gated entries
        qv[0] = 0; qv[0, 17] = 2.5                                # one-hot queries, gated and ungated
        qv[1] = 0; qv[1, d + 9] = 1.5
        qv[2] = 0                                                 # a zero query
        qv[3, :d] *= 300                                          # huge gated query values
        qv[4, d:] *= 300                                          # huge ungated query values
        qv[5:20] *= 0.3                                           # fp32 values that are not fp16-representable
        qv[20, :d] = qv[20, :d].abs() * -1                        # negative gated query values on a non-negative corpus
        cv = cv.half()
    ix = G.GipIndex(cv, ci)
    assert ix.info(_lib.INFO_GATED_I8) == (1 if mode == "gated_i8" else 0)
    qi16 = qi.to(torch.int16)
    qb, keep = _lib.make_query_batch(qv, qi16)
    margin = np.zeros(nq, np.float32)
    _lib.check(ix._lib.dhr_debug_query_margins(ix._h, C.byref(qb), margin.ctypes.data, None), "margins")
    mg = torch.from_numpy(margin).to(dev).double()
    cg, cd = cv[:, :d], cv[:, d:].double()
    worst = torch.full((nq,), float("inf"), dtype=torch.float64, device=dev)
    slab = min(250_000, n)                   # n is a multiple of it: the dump's leading dimension is the slab width
    out = torch.empty((nq, slab), dtype=torch.float32, device=dev)
    ex_keep = None
    for lo in range(0, n, slab):
        hi = min(n, lo + slab)
        _lib.check(ix._lib.dhr_debug_bound_scores(ix._h, C.byref(qb), lo, hi, out.data_ptr(), None), "debug_bound")
        ex = torch.empty((nq, hi - lo), dtype=torch.float64, device=dev)
        cgs, cis = cg[lo:hi].double(), ci[lo:hi].to(torch.int16)
        dense = qv[:, d:].double() @ cd[lo:hi].T
        for q in range(nq):
            ex[q] = (cgs * (cis == qi16[q][None, :])) @ qv[q, :d].double() + dense[q]
        worst = torch.minimum(worst, (out[:, :hi - lo].double() - ex + mg[:, None]).min(dim=1).values)
        if lo == 0:
            ex_keep = ex[:3, :5000].cpu().numpy()
    ix.close()
    # the torch float64 scores above are the oracle's (checked on a corner)
    c32 = cv[:5000].float().cpu().numpy(); cin = ci[:5000].cpu().numpy()
    for q in range(3):
        np.testing.assert_allclose(ex_keep[q], O.gip_scores_f64(qv[q].cpu().numpy(), qi16[q].cpu().numpy(), c32, cin), rtol=1e-9, atol=1e-9)
    w = worst.cpu().numpy()
    print("\n[%s / %s] minimum head room  U - (exact - margin)  over %d x %d pairs: %.3e (margins %.3e .. %.3e)" %
          (mode, kind, nq, n, w.min(), margin.min(), margin.max()))
    assert np.all(w >= 0.0), (w.min(), int(w.argmin()))


def _check_theta_mode(info, q, qi, c32, ci, rows, scores, ref_rows=None):
    """theta>0 modes against float64: one-stage = top-k of the stage-1 score; --rerank = the two-stage tie-band rule
    (stage-1 boundary at agip_topk, stage-2 boundary at topk).  Rows that differ from the reference's must lie in a band."""
    s1 = O.stage1_scores_f64(q, qi, c32, ci, info.get("theta", 0.1), info.get("IP", False))
    if info.get("rerank", False):
        ex = O.gip_scores_f64(q, qi, c32, ci)
        O.check_two_stage(rows, scores, s1, ex, info.get("agip_topk", 10000), info["topk"])
        if ref_rows is not None:
            rr = np.asarray(ref_rows)[np.argsort(-ex[np.asarray(ref_rows)], kind="stable")]
            O.check_two_stage(rr, ex[rr], s1, ex, info.get("agip_topk", 10000), info["topk"])   # the rule admits the reference
    else:
        O.check_topk(rows, scores, s1, info["topk"])
        if ref_rows is not None:
            rr = np.asarray(ref_rows)[np.argsort(-s1[np.asarray(ref_rows)], kind="stable")]
            O.check_topk(rr, s1[rr], s1, info["topk"])


FN_BRUTE = ["F1_bm25_brute", "F1b_mix8_brute", "F3_hyb_brute_k100", "F3_hyb_brute_k1000", "F4_hyb128_brute",
            "F5_hyb_lamda05", "F5_hyb_lamda03", "F7_hyb_shard0of3", "F7_hyb_shard1of3", "F7_hyb_shard2of3"]


@pytest.mark.parametrize("case", FN_BRUTE)
def test_gip_retrieval_golden(G, golden, case, gated_image):
    """GIP_retrieval (HIP) vs the reference's recorded rows/scores and vs the exact oracle."""
    info, ref_rows, ref_scores = golden.case(case)
    d = golden.inputs(info["inputs"])
    q, qi = O.prepare_queries(d["qv"], d["qi"], 768, info.get("lamda", 1.0))
    lo, hi = info.get("row_lo", 0), info.get("row_hi", d["cv"].shape[0])
    cv, ci = d["cv"][lo:hi], d["ci"][lo:hi]
    res, sc = G.GIP_retrieval(list(d["qids"]), q, qi, cv, ci, case_args(info))
    c32 = cv.astype(np.float32)
    for i, qid in enumerate(d["qids"]):
        ex = O.gip_scores_f64(q[i], qi[i], c32, ci)
        O.check_topk(res[qid], sc[qid], ex, info["topk"], ref_scores=ref_scores[i])
        diff = set(res[qid]) ^ set(ref_rows[i].tolist())
        if diff:       # only ties / fp32-noise at the boundary may differ from the reference
            kth = min(sc[qid])
            assert np.all(np.abs(ex[sorted(diff)] - kth) <= 1e-5 * max(1.0, abs(kth)))


def test_ip_retrieval_golden(G, golden):
    info, ref_rows, ref_scores = golden.case("F2_dense_ip")
    d = golden.inputs("dense")
    q, _ = O.prepare_queries(d["qv"], None, 768, 1.0)
    res, sc = G.IP_retrieval(list(d["qids"]), q, d["cv"], case_args(info))
    for i, qid in enumerate(d["qids"]):
        assert res[qid] == ref_rows[i].tolist()
        np.testing.assert_allclose(sc[qid], ref_scores[i], rtol=2e-6, atol=2e-6)


@pytest.mark.parametrize("case", ["F6_hyb_theta03_rerank", "F6_hyb_theta03_norerank", "F6_hyb_ip_rerank",
                                  "F6_hyb_ip_norerank"])
def test_theta_modes_golden(G, golden, case, gated_image):
    info, ref_rows, ref_scores = golden.case(case)
    d = golden.inputs("hyb")
    q, qi = O.prepare_queries(d["qv"], d["qi"], 768, 1.0)
    res, sc = G.GIP_retrieval(list(d["qids"]), q, qi, d["cv"], d["ci"], case_args(info))
    c32 = d["cv"].astype(np.float32)
    for i, qid in enumerate(d["qids"]):
        np.testing.assert_allclose(np.sort(sc[qid]), np.sort(ref_scores[i]), rtol=3e-6, atol=3e-6)
        _check_theta_mode(info, q[i], qi[i], c32, d["ci"], res[qid], sc[qid], ref_rows[i].tolist())


def test_k_larger_than_n(G, golden):
    d = golden.inputs("hyb")
    q, qi = O.prepare_queries(d["qv"], d["qi"], 768, 1.0)
    args = case_args(dict(topk=100, brute_force=True))
    with pytest.raises(RuntimeError, match="out of range"):
        G.GIP_retrieval(list(d["qids"]), q, qi, d["cv"][:64], d["ci"][:64], args)
    args.allow_short = True
    res, sc = G.GIP_retrieval(list(d["qids"]), q, qi, d["cv"][:64], d["ci"][:64], args)
    for i, qid in enumerate(d["qids"]):
        ex = O.gip_scores_f64(q[i], qi[i], d["cv"][:64].astype(np.float32), d["ci"][:64])
        assert len(res[qid]) == 64
        O.check_topk(res[qid], sc[qid], ex, 100)
    # IP_retrieval silently returns N rows, like the reference (F8)
    info, ref_rows, _ = golden.case("F8_ip_k_gt_n")
    dd = golden.inputs("dense")
    qd, _ = O.prepare_queries(dd["qv"], None, 768, 1.0)
    res, sc = G.IP_retrieval(list(dd["qids"]), qd, dd["cv"][:64], case_args(info))
    for i, qid in enumerate(dd["qids"]):
        assert res[qid] == ref_rows[i].tolist()


@pytest.mark.parametrize("cap,first,nb", [(1024, 0, 1), (4096, 2048, 2), (16384, 0, 0), (1024, 0, 2)])
def test_multi_phase_and_overflow(G, cap, first, nb, gated_image):
    """Small candidate capacity forces many bound-GEMM phases and overflow retries; results must not
    change.  N is ragged, K = 768+128."""
    from dhr_amd import _lib, synth
    cv, ci, qv, qi = synth.make_pair(7, 21000, 40, 768, 128)
    q32 = qv.astype(np.float32)
    _, _, st = _search_check(G, cv, ci, q32, qi, 100, params=[(_lib.PARAM_CAND_CAP, cap), (_lib.PARAM_FIRST_ROWS, first)],
                             queries=range(0, 40, 5), idx_buckets=nb)
    assert st["phases"] >= 2
    print(cap, first, st)


def test_negative_dlr_values_abs_mode(G):
    from dhr_amd import synth
    cv, ci, qv, qi = synth.make_pair(8, 6000, 16, 768, 64)
    rng = np.random.default_rng(0)
    cv = cv.copy(); qv = qv.copy()
    cv[:, :768] *= rng.choice([-1, 1], size=(6000, 768)).astype(np.float16)
    qv[:, :768] *= rng.choice([-1, 1], size=(16, 768)).astype(np.float16)
    _search_check(G, cv, ci, qv.astype(np.float32), qi, 50)
    _search_check(G, cv, ci, qv.astype(np.float32), qi, 50, idx_buckets=1)


def test_fp32_queries_not_fp16_representable(G):
    from dhr_amd import synth
    cv, ci, qv, qi = synth.make_pair(9, 5000, 8, 768, 768)
    q32 = qv.astype(np.float32)
    q32[:, 768:] *= np.float32(0.3)         # --lamda 0.3: not representable in fp16
    _search_check(G, cv, ci, q32, qi, 100)


def test_dense_only_and_bm25_int16(G):
    from dhr_amd import synth
    cv, _, qv, _ = synth.make_pair(10, 9000, 8, 0, 768, kind="dense")
    _search_check(G, cv, None, qv.astype(np.float32), None, 100)
    cv, ci, qv, qi = synth.make_pair(11, 9000, 8, 768, 0, kind="bm25")
    assert ci.dtype == np.int16
    _search_check(G, cv, ci, qv.astype(np.float32), qi, 100)
    _search_check(G, cv, ci, qv, qi, 100)   # fp16 queries straight from the file


def test_row_offset_and_score_rows(G):
    from dhr_amd import synth
    cv, ci, qv, qi = synth.make_pair(12, 3000, 8, 768, 128)
    q32 = qv.astype(np.float32)
    scores, rows, _ = _search_check(G, cv, ci, q32, qi, 64, row_offset=1_000_000)
    ix = G.GipIndex(cv, ci, row_offset=1_000_000)
    s2 = ix.score_rows(q32, qi, rows)
    np.testing.assert_array_equal(s2, scores)
    bad = rows.copy(); bad[:, 0] = -1; bad[:, 1] = 5      # outside the shard -> -inf
    s3 = ix.score_rows(q32, qi, bad)
    assert np.all(np.isneginf(s3[:, :2]))
    ix.close()


def test_device_inputs_and_outputs(G):
    import torch
    from dhr_amd import synth
    cv, ci, qv, qi = synth.make_pair(13, 4000, 8, 768, 128)
    ix_h = G.GipIndex(cv, ci)
    s_h, r_h = ix_h.search(qv.astype(np.float32), qi, 50)
    ix_h.close()
    ix_d = G.GipIndex(torch.from_numpy(cv).cuda(), torch.from_numpy(ci).cuda())
    s_d, r_d = ix_d.search(torch.from_numpy(qv).cuda(), torch.from_numpy(qi).cuda(), 50, out_device=True)
    ix_d.close()
    np.testing.assert_array_equal(s_d.cpu().numpy(), s_h)
    np.testing.assert_array_equal(r_d.cpu().numpy(), r_h)


def test_merge_topk_device_matches_host_and_oracle(G):
    import ctypes as C
    import torch
    from dhr_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(3)
    q, lists, k = 37, 4, 100
    s = np.round(rng.standard_normal((q, lists * k)).astype(np.float32), 1)      # many exact ties
    r = rng.permutation(10_000_000)[: q * lists * k].reshape(q, lists * k).astype(np.int64)
    r[:, -7:] = -1
    es, er = O.merge_topk([s], [r], k)
    hs, hr = np.empty((q, k), np.float32), np.empty((q, k), np.int64)
    _lib.check(lib.dhr_merge_topk_host(q, lists * k, s.ctypes.data, r.ctypes.data, k, hs.ctypes.data, hr.ctypes.data), "host merge")
    np.testing.assert_array_equal(hs, es); np.testing.assert_array_equal(hr, er)
    ds, dr = torch.from_numpy(s).cuda(), torch.from_numpy(r).cuda()
    os_, or_ = torch.empty((q, k), dtype=torch.float32, device="cuda"), torch.empty((q, k), dtype=torch.int64, device="cuda")
    _lib.check(lib.dhr_merge_topk(0, q, lists * k, ds.data_ptr(), dr.data_ptr(), k, os_.data_ptr(), or_.data_ptr(), 0), "dev merge")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(os_.cpu().numpy(), es); np.testing.assert_array_equal(or_.cpu().numpy(), er)


@pytest.mark.parametrize("n_lists,q,ll,k", [(8, 37, 192, 1000), (3, 5, 1000, 1000), (2, 4, 64, 10), (8, 3, 1024, 1000), (1, 3, 50, 80)])
def test_merge_sorted_lists_device(G, n_lists, q, ll, k):
    """dhr_merge_topk_lists (rank merge of sorted per-shard lists in all-gather layout) == host twin == oracle."""
    import torch
    from dhr_amd import _lib, dist as D
    from tests.util import sorted_lists
    lib = _lib.load()
    rng = np.random.default_rng(100 * n_lists + ll)
    s, r = sorted_lists(rng, n_lists, q, ll)
    es, er = O.merge_topk(list(s), list(r), k)
    ds, dr = torch.from_numpy(s).cuda(), torch.from_numpy(r).cuda()
    ms, mr = D.merge_sorted_lists(ds, dr, k)                       # wrapper (long lists go to the general reduce)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ms.cpu().numpy(), es)
    np.testing.assert_array_equal(mr.cpu().numpy(), er)
    ks, kr = torch.empty((q, k), dtype=torch.float32, device="cuda"), torch.empty((q, k), dtype=torch.int64, device="cuda")
    _lib.check(lib.dhr_merge_topk_lists(0, q, n_lists, ll, ds.data_ptr(), dr.data_ptr(), k, ks.data_ptr(), kr.data_ptr(), 0),
               "dhr_merge_topk_lists")                             # the rank-merge kernel itself, any shape that fits the LDS
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ks.cpu().numpy(), es)
    np.testing.assert_array_equal(kr.cpu().numpy(), er)
    hs, hr = D.merge_sorted_lists(torch.from_numpy(s), torch.from_numpy(r), k)       # host twin through the same wrapper
    np.testing.assert_array_equal(hs.numpy(), es)
    np.testing.assert_array_equal(hr.numpy(), er)
    # scores only (the shards' sample scores): the r-th best of the union
    full = np.where(r >= 0, s, -np.inf).astype(np.float32)
    rr = min(ll, 58)
    tau = D.common_threshold(torch.from_numpy(np.ascontiguousarray(full[:, :, :rr])).cuda(), rr).cpu().numpy()
    want = -np.sort(-full[:, :, :rr].transpose(1, 0, 2).reshape(q, -1), axis=1)[:, rr - 1]
    np.testing.assert_array_equal(tau, want)


def test_merge_sorted_lists_beyond_lds_falls_back_to_general_reduce(G):
    import torch
    from dhr_amd import dist as D
    from tests.util import sorted_lists
    s, r = sorted_lists(np.random.default_rng(9), 8, 2, 2000, ragged=False)          # 8*2000*12 B > 160 KiB
    es, er = O.merge_topk(list(s), list(r), 1000)
    ms, mr = D.merge_sorted_lists(torch.from_numpy(s).cuda(), torch.from_numpy(r).cuda(), 1000)
    np.testing.assert_array_equal(ms.cpu().numpy(), es)
    np.testing.assert_array_equal(mr.cpu().numpy(), er)


def test_sharded_equals_unsharded(G, gated_image):
    """Row shards (gip_retrieval.py:292-306 arithmetic) + the shard reduce == one index."""
    from dhr_amd import synth, _lib
    cv, ci, qv, qi = synth.make_pair(14, 10007, 16, 768, 128)
    q32 = qv.astype(np.float32)
    full_s, full_r, _ = _search_check(G, cv, ci, q32, qi, 100, queries=[0, 5])
    parts_s, parts_r = [], []
    for sh in range(3):
        lo, hi = G.shard_bounds(10007, 3, sh)
        ix = G.GipIndex(cv[lo:hi], ci[lo:hi], row_offset=lo)
        s, r = ix.search(q32, qi, 100)
        ix.close()
        parts_s.append(s); parts_r.append(r)
    ms, mr = O.merge_topk(parts_s, parts_r, 100)
    np.testing.assert_array_equal(mr, full_r)
    np.testing.assert_array_equal(ms, full_s)


@pytest.mark.parametrize("fname,argv", [
    ("golden_main_hyb_brute.trec", ["--brute_force", "--combine_cls", "--topk", "100"]),
    ("golden_main_hyb_lamda05.trec", ["--brute_force", "--topk", "100", "--lamda", "0.5", "--run_name", "dhr"]),
    ("golden_main_hyb_theta_rerank.trec", ["--theta", "0.3", "--rerank", "--agip_topk", "512", "--topk", "100"]),
    ("golden_main_hyb_shard1.trec", ["--brute_force", "--topk", "100", "--total_shrad", "3", "--shrad", "1"]),
    ("golden_main_hyb_shard2.trec", ["--brute_force", "--topk", "100", "--total_shrad", "3", "--shrad", "2"]),
])
def test_cli_main_trec(G, golden, fname, argv, gated_image):
    d = golden.inputs("hyb")
    mq = golden.inputs("main_queries")
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        qp, ip_ = os.path.join(tmp, "q.pt"), os.path.join(tmp, "i.pt")
        dump_pickle(qp, mq["qv"], mq["qi"], [str(x) for x in mq["qids"]])
        dump_pickle(ip_, d["cv"], d["ci"], [str(x) for x in d["docids"]])
        os.chdir(tmp)
        try:
            G.main(["--query_emb_path", qp, "--index_path", ip_] + argv)
            name = "result.trec" if "--total_shrad" not in argv else "result{}.trec".format(argv[-1])
            got = open(os.path.join(tmp, name)).read()
        finally:
            os.chdir(cwd)
    ref = parse_trec(golden.trec(fname))
    out = parse_trec(got)
    assert list(ref) == list(out)
    # float64 tie-band rule on the printed lists (the self-match filter of gip_retrieval.py:340 removed at most the
    # query's own row: it is put back at its rank before the check)
    opt = dict(zip(argv[::1], argv[1:] + [None]))
    info = dict(topk=int(opt["--topk"]), theta=float(opt.get("--theta", 0.1)), rerank="--rerank" in argv,
                agip_topk=int(opt.get("--agip_topk", 10000)), brute_force="--brute_force" in argv)
    lo, hi = O.shard_rows(len(d["docids"]), int(opt.get("--total_shrad", 1)), int(opt.get("--shrad", 0)))
    q, qi = O.prepare_queries(mq["qv"], mq["qi"], 768, float(opt.get("--lamda", 1.0)))
    c32, ci = d["cv"][lo:hi].astype(np.float32), d["ci"][lo:hi]
    row_of = {str(x): r for r, x in enumerate(d["docids"][lo:hi])}
    for i, qid in enumerate(str(x) for x in mq["qids"]):
        assert [x[1] for x in ref[qid]] == [x[1] for x in out[qid]]
        np.testing.assert_allclose([x[2] for x in ref[qid]], [x[2] for x in out[qid]], rtol=3e-6, atol=3e-6)
        ex = O.gip_scores_f64(q[i], qi[i], c32, ci)
        for lst in (out[qid], ref[qid]):          # the rule must hold for the build's file AND admit the reference's
            rows = [row_of[x[0]] for x in lst]
            ranks = [x[1] for x in lst]
            if len(rows) < info["topk"]:           # own row filtered: rank numbers keep the gap
                gap = next((j for j, rk in enumerate(ranks) if rk != j + 1), len(rows))
                rows.insert(gap, row_of[qid])
            rows = np.asarray(rows)
            if info["brute_force"]:
                O.check_topk(rows, -np.sort(-ex[rows]), ex, info["topk"])
            else:
                _check_theta_mode(info, q[i], qi[i], c32, ci, rows, -np.sort(-ex[rows]))
        got_scores = np.asarray([x[2] for x in out[qid]])
        np.testing.assert_allclose(got_scores, ex[[row_of[x[0]] for x in out[qid]]], rtol=0, atol=1e-3)


def test_cli_dense_merged_index(G, golden):
    """index.py merge (dense: index array -> 0) then gip main() on it -> IP_retrieval path."""
    from dhr_amd.retrieval import index as I
    dd = golden.inputs("dense")
    b = golden.meta["index_merge"]["bounds"]
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(3):
            dump_pickle(os.path.join(tmp, f"msmarco-passage.split{i:02d}.pt"), dd["cv"][b[i]:b[i + 1]], None,
                        [str(x) for x in dd["docids"][b[i]:b[i + 1]]])
        I.main(["--index_path", tmp])
        qp = os.path.join(tmp, "q.pt")
        dump_pickle(qp, dd["qv"], None, [str(x) for x in dd["qids"]])
        os.chdir(tmp)
        try:
            G.main(["--query_emb_path", qp, "--index_path", os.path.join(tmp, "msmarco-passage.index.pt"), "--topk", "100"])
            got = open(os.path.join(tmp, "result.trec")).read()
        finally:
            os.chdir(cwd)
    ref = parse_trec(golden.trec("golden_main_dense_merged.trec"))
    out = parse_trec(got)
    for qid in ref:      # row order differs (sorted merge) but docids/scores are the same
        assert [x[0] for x in ref[qid]] == [x[0] for x in out[qid]]
        np.testing.assert_allclose([x[2] for x in ref[qid]], [x[2] for x in out[qid]], rtol=3e-6, atol=3e-6)


def test_larger_random_hybrid(G, gated_image):
    """N = 200k x 1536, 300 queries (two query tiles), k = 1000; a sample of queries is checked
    against the exact oracle."""
    from dhr_amd import synth
    cv, ci, qv, qi = synth.make_pair(15, 200_000, 300, 768, 768)
    _, _, st = _search_check(G, cv, ci, qv.astype(np.float32), qi, 1000, queries=[0, 1, 150, 299])
    print(st)


def _structured_corpus(n, boosted_mod, period=16, head_tiles=0):   # head: no exhaustive rows in a sampled search since round 5 (threshold bootstrap, api.hip search_core); 1 tile until round 4
    """Dense-only corpus whose best rows all sit in tiles with (tile - head) % period == boosted_mod."""
    rng = np.random.default_rng(5)
    cv = (rng.standard_normal((n, 64)) * 0.05).astype(np.float16)
    tile = np.arange(n) // 256
    boosted = (tile >= head_tiles) & (((tile - head_tiles) % period) == boosted_mod)
    cv[boosted, 0] += np.float16(2.0)
    qv = np.zeros((5, 64), np.float16)
    qv[:, 0] = 1.0
    qv[:, 1:] = (rng.standard_normal((5, 63)) * 0.05).astype(np.float16)
    return cv, qv


@pytest.mark.parametrize("boosted_mod", [0, 3])
def test_sampled_threshold_fallbacks(G, boosted_mod, gated_image):
    """Adversarial row order for the sampled threshold: (0) every high-scoring row sits in a SAMPLE tile,
    so tau_hat is far too high and fewer than k rows reach it -> the queries must be redone exactly;
    (3) every high-scoring row sits in one non-sample residue -> tau_hat is low, lists overflow.
    Either way the result must equal the exact top-k."""
    from dhr_amd import _lib
    n = 300_000
    cv, qv = _structured_corpus(n, boosted_mod)
    _, _, st = _search_check(G, cv, None, qv.astype(np.float32), None, 1000,
                             params=[(_lib.PARAM_CAND_CAP, 4096), (_lib.PARAM_SAMPLE_PERIOD, 16)])   # the corpus is built for period 16
    print(boosted_mod, st)
    if boosted_mod == 0:
        assert st["sample_fallback_queries"] == 5       # all 5 fail at depth 0 (no list overflowed) and go straight to the plain streaming pass
    _, _, st2 = _search_check(G, cv, None, qv.astype(np.float32), None, 1000,
                              params=[(_lib.PARAM_SAMPLE_PERIOD, 0)])
    assert st2["sample_fallback_queries"] == 0


def test_sampling_on_off_same_result(G):
    from dhr_amd import _lib, synth
    cv, ci, qv, qi = synth.make_pair(16, 150_000, 20, 768, 128)
    q32 = qv.astype(np.float32)
    out = []
    for period in (0, 8, 16):
        ix = G.GipIndex(cv, ci)
        ix.set_param(_lib.PARAM_SAMPLE_PERIOD, period)
        s, r = ix.search(q32, qi, 500)
        out.append((s, r, ix.stats()))
        ix.close()
    for s, r, st in out[1:]:
        np.testing.assert_array_equal(r, out[0][1])
        np.testing.assert_array_equal(s, out[0][0])
    print([o[2]["candidates_exact"] for o in out], [o[2]["phases"] for o in out])


@pytest.mark.parametrize("k", [4097, 10000, 16384, 16385, 30000])
def test_large_k(G, k):
    """k beyond the single-pass LDS merge (the documented --agip_topk default is 10000) and beyond the LDS altogether
    (k > 16384: global-memory merge, select_global.hip; the reference's torch.topk takes any k)."""
    from dhr_amd import synth
    cv, ci, qv, qi = synth.make_pair(17, 40_000, 6, 768, 64)
    _search_check(G, cv, ci, qv.astype(np.float32), qi, k, queries=[0, 5])


@pytest.mark.parametrize("order", ["ascending", "descending", "blocks"])
def test_large_k_adversarial_row_order(G, order):
    """The running list of 4 096 < k <= 16 384 is merged in place in memory (select_big_kernel).  Scores that RISE with the row id make
    every batch of every phase beat the whole list (each merge moves all of it), scores that fall leave it untouched after the first
    phases, alternating blocks interleave old and new keys; many rows tie (score desc, row asc decides)."""
    from dhr_amd import synth
    n, k = 60_000, 9000
    cv, ci, qv, qi = synth.make_pair(61, n, 3, 768, 64)
    r = np.arange(n, dtype=np.float32) / n
    ramp = r if order == "ascending" else (1.0 - r) if order == "descending" else ((np.arange(n) // 997) % 2).astype(np.float32) * 0.5 + 0.25 * r
    cv = cv.copy(); qv = qv.copy()
    cv[:, -1] = (4.0 * ramp).astype(np.float16)               # one ungated column carries the order; fp16 steps: runs of tied rows
    qv[:, -1] = np.float16(3.0)
    _search_check(G, cv, ci, qv.astype(np.float32), qi, k)


def test_two_stage_default_agip_topk(G):
    """--theta 0.3 --rerank with the reference's default --agip_topk 10000 against the oracle."""
    from dhr_amd import synth
    cv, ci, qv, qi = synth.make_pair(18, 30_000, 4, 768, 128)
    q32 = qv.astype(np.float32)
    args = case_args(dict(topk=1000, theta=0.3, rerank=True, agip_topk=10000))
    qids = [str(i) for i in range(4)]
    res, sc = G.GIP_retrieval(qids, q32, qi, cv, ci, args)
    eres, esc = O.GIP_retrieval(qids, q32, qi, cv.astype(np.float32), ci, args)
    c32 = cv.astype(np.float32)
    for i, qid in enumerate(qids):
        np.testing.assert_allclose(np.sort(sc[qid]), np.sort(esc[qid]), rtol=3e-6, atol=3e-6)
        _check_theta_mode(dict(topk=1000, theta=0.3, rerank=True, agip_topk=10000), q32[i], qi[i], c32, ci, res[qid], sc[qid], eres[qid])


@pytest.mark.parametrize("mode,k1,k", [("theta", 512, 100), ("ip", 300, 300), ("theta", 5000, 1000)])
def test_search_rerank_device_equals_composed(G, mode, k1, k):
    """dhr_search_rerank (both stages on the device) == dhr_search + dhr_score_rows + host top-k,
    and stage 2 == the oracle's exact GIP on the stage-1 rows (gip_retrieval.py:141-153)."""
    from dhr_amd import synth
    cv, ci, qv, qi = synth.make_pair(23, 30000, 24, 768, 128)
    q = qv.astype(np.float32)
    ix = G.GipIndex(cv, ci)
    try:
        if mode == "theta":
            q1, qi1 = np.where(q > 0.3, q, np.float32(0)), qi
        else:
            q1, qi1 = q, None
        s1, r1 = ix.search(q1, qi1, k1)
        s2 = ix.score_rows(q, qi, r1)
        order = np.lexsort((r1, -s2.astype(np.float64)), axis=1)[:, :k]
        rows_c = np.take_along_axis(r1, order, axis=1)
        sc_c = np.take_along_axis(s2, order, axis=1)
        sc_d, rows_d = ix.search_rerank(q1, qi1, q, qi, k1, k)
        np.testing.assert_array_equal(rows_d, rows_c)
        np.testing.assert_array_equal(sc_d, sc_c)
        for i in range(0, 24, 5):
            ex = O.gip_scores_f64(q[i], qi[i], cv[r1[i]].astype(np.float32), ci[r1[i]])
            np.testing.assert_allclose(sc_d[i], np.sort(ex)[::-1][:k], rtol=2e-6, atol=2e-6)
    finally:
        ix.close()


def test_config1_bm25_100k(G):
    """BASELINE config 1 shape: DLR-only BM25-like vectors, int16 slice index, 100k passages."""
    from dhr_amd import synth
    cv, ci, qv, qi = synth.make_pair(19, 100_000, 48, 768, 0, kind="bm25")
    _, _, st = _search_check(G, cv, ci, qv.astype(np.float32), qi, 1000, queries=[0, 13, 47])
    print(st)


@pytest.mark.parametrize("nb", [0, 1, 2])
def test_negative_query_values_on_nonneg_corpus(G, nb):
    """Corpus gated values >= 0 (no |.| mode) but the QUERY carries negative gated values: the bound
    operand must clamp them (q+ d >= gated q d), else rows would be lost."""
    from dhr_amd import synth
    cv, ci, qv, qi = synth.make_pair(20, 8000, 8, 768, 64)
    rng = np.random.default_rng(1)
    qv = qv.copy()
    qv[:, :768] *= rng.choice([-1, 1], size=(8, 768)).astype(np.float16)
    _search_check(G, cv, ci, qv.astype(np.float32), qi, 100, idx_buckets=nb)


def _fake_world_search(G, shards, q32, qi, k, mid=False):
    """dist.sharded_search with the collectives replaced by in-process tensor ops (one GPU, S shards); mid: with the second threshold
    agreement (dhr_search_mid) between begin and finish."""
    import torch
    from dhr_amd import dist as D
    from dhr_amd import _lib
    for s in shards:
        s.set_param(_lib.PARAM_SAMPLE_SHARE, len(shards))
    r = shards[0].sample_rank(k)
    assert r > 0 and all(s.sample_rank(k) == r for s in shards)
    samples = [s.search_begin(q32, qi, k) for s in shards]
    tau = D.common_threshold(torch.stack(samples), shards[0].union_rank(k))
    if mid:
        ranks = [s.mid_ranks(k) for s in shards]
        assert all(a > 0 and b > 0 for a, b in ranks), ranks
        rl, ru = max(a for a, _ in ranks), max(b for _, b in ranks)
        seen = [s.search_mid(tau, rl) for s in shards]
        tau2 = D.common_threshold(torch.stack(seen), min(ru, len(shards) * rl))
        tau = torch.maximum(tau, tau2)
    outs = [s.search_finish(tau) for s in shards]
    count = torch.stack([o[2] for o in outs])
    tot = count.clamp(min=0).sum(0)
    failed = torch.nonzero((tot < k) | (count < 0).any(0)).flatten()
    scores = [o[0] for o in outs]
    rows = [o[1] for o in outs]
    if failed.numel():
        ids = failed.cpu().numpy()
        for i, s in enumerate(shards):
            fs, fr = s.search(q32[ids], None if qi is None else qi[ids], k, out_device=True)
            scores[i][failed] = fs
            rows[i][failed] = fr
    ms, mr = D.merge_topk(torch.cat(scores, 1), torch.cat(rows, 1), k)
    return ms.cpu().numpy(), mr.cpu().numpy(), int(failed.numel()), [int(x) for x in tot[:4]]


def test_smaller_batch_reuses_the_workspace(G):
    """A batch with fewer queries runs in the buffers of the larger one before it (ensure_ws: until round 4 every change of the batch size freed
    and re-allocated the workspace -- 0.7 s for the one-query repair step of a sharded search at full size): the device footprint does not move,
    the padded query rows of the smaller batch (stale rows of the larger one) stay out of the results, and the larger batch still answers the same."""
    from dhr_amd import synth
    cv, ci, qv, qi = synth.make_pair(41, 60_000, 300, 768, 64)
    q = qv.astype(np.float32)
    ix = G.GipIndex(cv, ci)
    try:
        s_all, r_all = ix.search(q, qi, 100)
        bytes_all = ix.device_bytes()
        for sub in (np.array([7]), np.arange(250, 263), np.arange(0, 300, 7)):
            s_sub, r_sub = ix.search(q[sub], qi[sub], 100)
            assert ix.device_bytes() == bytes_all
            np.testing.assert_array_equal(r_sub, r_all[sub])
            np.testing.assert_array_equal(s_sub, s_all[sub])
        s2, r2 = ix.search(q, qi, 100)
        assert ix.device_bytes() == bytes_all
        np.testing.assert_array_equal(r2, r_all)
        np.testing.assert_array_equal(s2, s_all)
        for i in (0, 150, 299):
            ex = O.gip_scores_f64(q[i], qi[i], cv.astype(np.float32), ci)
            order = np.lexsort((np.arange(len(ex)), -ex))[:100]
            np.testing.assert_array_equal(r_all[i], order)
    finally:
        ix.close()


@pytest.mark.parametrize("stride", [1024, 4096])
def test_two_tier_candidate_lists(G, gated_image, stride):
    """Two-tier bound lists (round 5: every query owns DHR_PARAM_LIST_STRIDE uniform slots, a hot query the rest of its depth from an arena
    planned on the device).  With a stride far below what the lists of this batch hold (1 024, the smallest admitted: below even the first sampled phase's; 4 096), the second tier carries most entries of the hot
    queries -- and a query whose plan came out too small overflows, is flagged and redone: either way the result must be the result of the
    default stride, which is checked against the oracle.  The footprint shrinks with the stride."""
    from dhr_amd import synth, _lib
    cv, ci, qv, qi = synth.make_pair(91, 300_000, 640, 768, 64)
    q = qv.astype(np.float32)
    q[:40, :768] *= 3.0                               # a few HOT queries: their lists are several times the average
    k = 200
    ix = G.GipIndex(cv, ci)
    try:
        ix.set_param(_lib.PARAM_PROFILE, 1)
        s0, r0 = ix.search(q, qi, k)
        st0, b0 = ix.stats(), ix.device_bytes()
        ix.set_param(_lib.PARAM_LIST_STRIDE, stride)
        s1, r1 = ix.search(q, qi, k)
        st1, b1 = ix.stats(), ix.device_bytes()
        np.testing.assert_array_equal(r1, r0)
        np.testing.assert_array_equal(s1, s0)
        s2, r2 = ix.search(q[5:9], qi[5:9], k)         # a smaller batch in the same workspace
        np.testing.assert_array_equal(r2, r0[5:9])
        print("\n[stride %d, gated image %s] bound %.0f -> exact %.0f per query, redone %d (default stride: %.0f -> %.0f, redone %d); device bytes %.2f -> %.2f GB"
              % (stride, gated_image, st1["candidates_bound"] / 640, st1["candidates_exact"] / 640, st1["sample_fallback_queries"],
                 st0["candidates_bound"] / 640, st0["candidates_exact"] / 640, st0["sample_fallback_queries"], b0 / 1e9, b1 / 1e9))
        if st1["sample_fallback_queries"] == 0:          # (a redone query brings the fallback workspace with its 16 x deeper lists)
            assert b1 < b0
        assert st1["sample_fallback_queries"] <= 64      # the plan (2 x the previous phase's rate + 2 048) covers all but a few queries
        c32 = cv.astype(np.float32)
        for i in (0, 3, 39, 40, 333, 639):
            ex = O.gip_scores_f64(q[i], qi[i], c32, ci)
            O.check_topk(r1[i], s1[i], ex, k)
    finally:
        ix.close()


@pytest.mark.parametrize("aux_cus,exclusive", [(64, 0), (128, 1)])
def test_two_tier_lists_with_cu_masked_streams(G, aux_cus, exclusive):
    """DHR_PARAM_AUX_CUS / DHR_PARAM_GEMM_EXCLUSIVE put the main pass' bound GEMM and its refine / rescoring on CU-masked streams of their own;
    both must enter the pass BEHIND the kernel that plans the second tier of the bound lists (until round 5 they waited on an event recorded
    before it: a GEMM that spilled past the uniform stride could pair a new ovf_cap with an old ovf_off -- the round-5 advisor's finding).  A
    small stride, hot queries, CU masks on: the result is the default configuration's, bit for bit, and no query is lost silently."""
    from dhr_amd import synth, _lib
    cv, ci, qv, qi = synth.make_pair(92, 300_000, 640, 768, 64)
    q = qv.astype(np.float32)
    q[:40, :768] *= 3.0
    k = 200
    ix = G.GipIndex(cv, ci)
    try:
        s0, r0 = ix.search(q, qi, k)
        ix.set_param(_lib.PARAM_LIST_STRIDE, 1024)
        ix.set_param(_lib.PARAM_AUX_CUS, aux_cus)
        ix.set_param(_lib.PARAM_GEMM_EXCLUSIVE, exclusive)
        for _ in range(3):                                 # (the plan of a step reads what the previous one left in the workspace)
            s1, r1 = ix.search(q, qi, k)
            np.testing.assert_array_equal(r1, r0)
            np.testing.assert_array_equal(s1, s0)
        c32 = cv.astype(np.float32)
        for i in (0, 39, 333):
            O.check_topk(r1[i], s1[i], O.gip_scores_f64(q[i], qi[i], c32, ci), k)
    finally:
        ix.close()


def test_allocation_failures_with_a_device(G):
    """The exception barrier with a device behind it (tests/test_abi_guard.py is the CPU part): every host allocation of dhr_index_create and of
    dhr_search fails once -- `new dhr_index()`, the std::vectors of the index build and of the controller, the event lists -- and each call
    comes back with DHR_ERR_NOMEM and a message; nothing unwinds through ctypes, the handle stays usable, the result is unchanged."""
    import ctypes as C
    from dhr_amd import synth, _lib
    lib = _lib.load()
    cv, ci, qv, qi = synth.make_pair(93, 70_000, 24, 768, 64)
    q = qv.astype(np.float32)
    k = 50
    d = _lib.IndexDesc(0, _lib.MEM_HOST, cv.shape[0], 768, 64, cv.ctypes.data, cv.shape[1], ci.ctypes.data, _lib.idx_code(ci.dtype), 0, ci.shape[1], 0)

    def create():
        h = C.c_void_p()
        rc = lib.dhr_index_create(C.byref(d), C.byref(h))
        return rc, h
    a0 = lib.dhr_debug_fail_alloc(0)
    rc, h = create()
    assert rc == 0
    n_create = lib.dhr_debug_fail_alloc(0) - a0
    assert n_create >= 3
    for i in range(1, n_create + 1):
        lib.dhr_debug_fail_alloc(i)
        rc, hh = create()
        lib.dhr_debug_fail_alloc(0)
        assert rc == _lib.ERR_NOMEM and not hh.value, (i, rc, lib.dhr_last_error())
    qb, keep = _lib.make_query_batch(q, qi)
    s0, r0 = np.zeros((24, k), np.float32), np.zeros((24, k), np.int64)
    s1, r1 = np.zeros((24, k), np.float32), np.zeros((24, k), np.int64)
    lib.dhr_index_set_param(h, _lib.PARAM_PROFILE, 1)       # (the timers allocate too)
    assert lib.dhr_search(h, C.byref(qb), k, s0.ctypes.data, r0.ctypes.data, _lib.MEM_HOST, None) == 0      # warm: the workspace exists
    a0 = lib.dhr_debug_fail_alloc(0)
    assert lib.dhr_search(h, C.byref(qb), k, s0.ctypes.data, r0.ctypes.data, _lib.MEM_HOST, None) == 0
    n_search = lib.dhr_debug_fail_alloc(0) - a0
    assert n_search >= 3
    for i in range(1, n_search + 1):
        lib.dhr_debug_fail_alloc(i)
        rc = lib.dhr_search(h, C.byref(qb), k, s1.ctypes.data, r1.ctypes.data, _lib.MEM_HOST, None)
        lib.dhr_debug_fail_alloc(0)
        assert rc == _lib.ERR_NOMEM and b"memory" in lib.dhr_last_error(), (i, rc, lib.dhr_last_error())
        assert lib.dhr_search(h, C.byref(qb), k, s1.ctypes.data, r1.ctypes.data, _lib.MEM_HOST, None) == 0      # the handle is usable right away
        np.testing.assert_array_equal(r1, r0)
        np.testing.assert_array_equal(s1, s0)
    print("\n[host allocations: dhr_index_create %d, dhr_search %d -- each failed once]" % (n_create, n_search))
    c32 = cv.astype(np.float32)
    for i in (0, 23):
        O.check_topk(r0[i], s0[i], O.gip_scores_f64(q[i], qi[i], c32, ci), k)
    lib.dhr_index_destroy(h)
    del keep


@pytest.mark.parametrize("mid", [False, True])
@pytest.mark.parametrize("kind", ["hybrid", "dense"])
def test_staged_sharded_search_common_threshold(G, kind, gated_image, mid):
    """Shards exchange their sample scores, agree on one threshold per query, and the union of their
    (now much shorter) lists still equals the unsharded exact result."""
    from dhr_amd import synth, _lib
    n, k, ns = 400_000, 1000, 4
    if kind == "hybrid":
        cv, ci, qv, qi = synth.make_pair(22, n, 12, 768, 64)
    else:
        cv, ci, qv, qi = synth.make_pair(23, n, 12, 0, 256, kind="dense")
    q32 = qv.astype(np.float32)
    full = G.GipIndex(cv, ci)
    fs, fr = full.search(q32, qi, k)
    full.close()
    shards = []
    for sh in range(ns):
        lo, hi = G.shard_bounds(n, ns, sh)
        shards.append(G.GipIndex(cv[lo:hi], None if ci is None else ci[lo:hi], row_offset=lo))
        shards[-1].set_param(_lib.PARAM_SAMPLE_PERIOD, 4)          # 100k-row shards: sample every 4th tile
    ms, mr, n_failed, tot = _fake_world_search(G, shards, q32, qi, k, mid=mid)
    exact_per_shard = [s.stats()["candidates_exact"] for s in shards]
    for s in shards:
        s.close()
    np.testing.assert_array_equal(mr, fr)
    np.testing.assert_array_equal(ms, fs)
    print(kind, "mid" if mid else "plain", "failed", n_failed, "counts>=tau", tot, "rows rescored per shard and query", [e // 12 for e in exact_per_shard])


@pytest.mark.parametrize("mid", [False, True])
def test_staged_sharded_search_failure_path(G, mid):
    """All high-scoring rows sit in sample tiles of shard 0: the common threshold is too high for the
    union to reach k rows, the count check must catch it and the local fallback must repair it."""
    from dhr_amd import _lib
    n, k, ns = 401_408, 1000, 2          # shard 1 starts on a multiple of 16 tiles: the boosted tiles are sample tiles of BOTH shards
    cv, qv = _structured_corpus(n, 0)
    q32 = qv.astype(np.float32)
    full = G.GipIndex(cv, None)
    fs, fr = full.search(q32, None, k)
    full.close()
    shards = []
    for sh in range(ns):
        lo, hi = G.shard_bounds(n, ns, sh)
        shards.append(G.GipIndex(cv[lo:hi], None, row_offset=lo))
        shards[-1].set_param(_lib.PARAM_SAMPLE_PERIOD, 16)         # the period the corpus is structured for
    ms, mr, n_failed, tot = _fake_world_search(G, shards, q32, None, k, mid=mid)
    for s in shards:
        s.close()
    assert n_failed == 5
    np.testing.assert_array_equal(mr, fr)
    np.testing.assert_array_equal(ms, fs)


@pytest.mark.parametrize("kind", ["hybrid", "dense", "hybrid3"])
def test_device_index_file_round_trip(G, tmp_path, kind):
    """dhr_index_save -> dhr_index_load: the loaded index answers bit-identically, the docid blob
    survives, row_offset can be overridden, a file of another format version is refused."""
    import ctypes as C
    from dhr_amd import _lib, synth
    d_dlr = 0 if kind == "dense" else 768
    if d_dlr:
        cv, ci, qv, qi = synth.make_pair(31, 5000, 16, d_dlr, 128)
    else:
        rng = np.random.default_rng(31)
        cv, qv = (rng.standard_normal((5000, 768)) * 0.1).astype(np.float16), (rng.standard_normal((16, 768)) * 0.1).astype(np.float16)
        ci = qi = None
    q = qv.astype(np.float32)
    docids = ["D%d" % i for i in range(5000)]
    ix = G.GipIndex(cv, ci, row_offset=1000, idx_buckets=1 if kind == "hybrid3" else 0)
    path = str(tmp_path / "corpus.dhr")
    try:
        s0, r0 = ix.search(q, qi, 100)
        ix.save(path, docids)
    finally:
        ix.close()
    assert G.GipIndex.is_device_file(path)
    ix2, ids2 = G.GipIndex.load(path)
    try:
        assert ids2 == docids and ix2.n_rows == 5000 and ix2.row_offset == 1000 and ix2.d_dlr == d_dlr
        s1, r1 = ix2.search(q, qi, 100)
        np.testing.assert_array_equal(r1, r0)
        np.testing.assert_array_equal(s1, s0)
        sc = ix2.score_rows(q, qi, r1[:, :7])
        np.testing.assert_array_equal(sc, s0[:, :7])
    finally:
        ix2.close()
    ix3, _ = G.GipIndex.load(path, row_offset=0)
    try:
        _, r3 = ix3.search(q, qi, 100)
        np.testing.assert_array_equal(r3, r0 - 1000)
    finally:
        ix3.close()
    raw = bytearray(open(path, "rb").read(4096))
    raw[8:12] = (77).to_bytes(4, "little")                           # version field of the header
    with open(path, "r+b") as f:
        f.write(raw)
    with pytest.raises(_lib.DhrError, match="file format version 77"):
        G.GipIndex.load(path)


def test_cli_device_index_file(G, golden, tmp_path, monkeypatch):
    """main(): --save_device_index writes the file, a second run with it as --index_path gives the same TREC run."""
    import pickle
    d = golden.inputs("hyb")
    monkeypatch.chdir(tmp_path)
    with open("q.pt", "wb") as f:
        pickle.dump([d["qv"], d["qi"], list(d["qids"])], f, protocol=4)
    with open("c.pt", "wb") as f:
        pickle.dump([d["cv"], d["ci"], list(d["docids"])], f, protocol=4)
    common = ["--query_emb_path", "q.pt", "--emb_dim", "768", "--brute_force", "--topk", "50"]
    G.main(common + ["--index_path", "c.pt", "--output", "a.trec", "--save_device_index", "c.dhr"])
    G.main(common + ["--index_path", "c.dhr", "--output", "b.trec"])
    assert open("a.trec").read() == open("b.trec").read() and len(open("a.trec").read()) > 1000


def test_densify_golden_and_random(G):
    """dhr_densify == the reference's recorded outputs and the oracle: values bit-exact, first maximum wins,
    numpy (host) and torch (device) inputs, fp16 / fp32, direct write into an index record, error messages."""
    import os
    import torch
    from dhr_amd import densify as DZ
    from oracle import densify_oracle as DO
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "densify_golden.npz"))
    for name, kw in (("a", dict(dims=768)), ("b", dict(dims=8, remove_dims=3)), ("c", dict(dims=16, remove_dims=0))):
        v, i = DZ.densify(g[name + "_in"], **kw)
        np.testing.assert_array_equal(v, g[name + "_val"])
        np.testing.assert_array_equal(i, g[name + "_idx"])
        assert v.dtype == g[name + "_val"].dtype and i.dtype == np.int64
        tv, ti = DZ.densify(torch.from_numpy(g[name + "_in"]).cuda(), **kw)
        np.testing.assert_array_equal(tv.cpu().numpy(), g[name + "_val"])
        np.testing.assert_array_equal(ti.cpu().numpy(), g[name + "_idx"])
        assert ti.dtype == torch.int64 and tv.is_cuda
    rng = np.random.default_rng(5)
    x = rng.standard_normal((513, 30522)).astype(np.float32)
    x[:, ::7] = np.float32(0.25)                                       # many exact ties
    ev, ei = DO.densify(x)
    v, i = DZ.densify(x)
    np.testing.assert_array_equal(v, ev)
    np.testing.assert_array_equal(i, ei)
    # the encoder driver's layout: fp16 values into the first 768 columns of a [B, 768+128] record, uint8 groups
    rec_v = np.zeros((513, 896), np.float16)
    rec_i = np.zeros((513, 768), np.uint8)
    DZ.densify_into(x, rec_v, rec_i)
    e16, e8 = DO.densify_encoded(x)
    np.testing.assert_array_equal(rec_v[:, :768], e16)
    np.testing.assert_array_equal(rec_i, e8)
    assert not rec_v[:, 768:].any()
    xd = torch.from_numpy(x).cuda().half()
    dv = torch.zeros((513, 896), dtype=torch.float16, device="cuda")
    di = torch.zeros((513, 768), dtype=torch.uint8, device="cuda")
    DZ.densify_into(xd, dv, di)
    h16, h8 = DO.densify_encoded(x.astype(np.float16))
    np.testing.assert_array_equal(dv[:, :768].cpu().numpy(), h16)
    np.testing.assert_array_equal(di.cpu().numpy(), h8)
    errs = list(g["errors"])
    with pytest.raises(ValueError) as e:
        DZ.densify(np.zeros((2, 3, 4), np.float32), dims=4, remove_dims=0)
    assert str(e.value) == errs[0]
    with pytest.raises(ValueError) as e:
        DZ.densify(np.zeros((2, 30), np.float32), dims=7, remove_dims=1)
    assert str(e.value) == errs[1]
    # throughput note (HBM-bound: every input byte once)
    big = torch.randn((4096, 30522), device="cuda")
    bv = torch.empty((4096, 768), dtype=torch.float16, device="cuda")
    bi = torch.empty((4096, 768), dtype=torch.uint8, device="cuda")
    DZ.densify_into(big, bv, bi)
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(5):
        DZ.densify_into(big, bv, bi)
    t1.record(); torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / 5
    print("densify 4096 x 30522 fp32: %.3f ms, %.2f TB/s" % (ms, 4096 * 29952 * 4 / ms / 1e9))


def test_pq_first_stage(G, tmp_path, monkeypatch):
    """--PQIP (parity with faiss UNPINNED): encode / decode / ADC search exact against the oracle with the same
    codebooks; the trained codebooks quantise as well as the oracle's k-means; recall of the first stage and the final
    top-k after the exact rerank against the brute-force search; CLI round trip."""
    import pickle
    from dhr_amd import synth
    from dhr_amd.retrieval import quantize_index as QI
    from oracle import pq_oracle as PO
    cv, ci, qv, qi = synth.make_pair(41, 20000, 16, 768, 128)            # d = 896, M = 64 -> dsub = 14
    q = qv.astype(np.float32)
    cb, codes, err = QI.train_and_encode(cv, 64, 8, iters=8)
    assert cb.shape == (64, 256, 14) and codes.shape == (20000, 64) and codes.dtype == np.uint8
    # encoding == oracle encoding under the same codebooks (ties aside)
    ecodes = PO.encode(cv[:3000].astype(np.float32), cb)
    assert (ecodes != codes[:3000]).mean() < 2e-3
    # training quality: within 3 % of the oracle's k-means with the same schedule (float summation order differs)
    ocb = PO.train(cv, 64, iters=8)
    assert PO.mse(cv[:4000], cb) <= 1.03 * PO.mse(cv[:4000], ocb)
    assert abs(err - PO.mse(cv[::max(1, 20000 // 65536)], cb)) <= 0.02 * err + 1e-6
    # decode == oracle decode (rounded to fp16)
    dec = QI.decode(cb, codes)
    np.testing.assert_array_equal(dec, PO.decode(codes, cb).astype(np.float16))
    # ADC scan (dhr_pq_*): the codes stay resident at 64 B per row; raw scores == the oracle's table-based ADC scores to 1e-5
    # (fp32 tables and sums; no fp16 rounding of a reconstruction), the search == the exact top-k of those scores
    pix = QI.PqIndex(cb, codes)
    ix = G.GipIndex(cv, ci)
    try:
        adc = PO.adc_scores(q, codes, cb)
        raw = pix.adc_scores(q).cpu().numpy()
        np.testing.assert_allclose(raw, adc, rtol=0, atol=1e-5 * max(1.0, float(np.abs(adc).max())))
        assert pix.device_bytes() - 64 * 256 * 14 * 4 >= 20000 * 64
        s1, r1 = pix.search(q, 500)
        assert pix.device_bytes() < 20000 * 64 + 64 * 256 * 14 * 4 + (1 << 30)       # codes + codebooks + the (bounded) search workspace
        for i in range(16):
            O.check_topk(r1[i], s1[i], adc[i], 500, atol=1e-4)
        s1d, r1d = pix.search(__import__("torch").from_numpy(qv).cuda(), 500, out_device=True)      # fp16 device batch
        np.testing.assert_array_equal(r1d.cpu().numpy(), r1)
        sk, rk = pix.search(q[:3], 16384)                                             # k at the limit, > the first scan block
        for i in range(3):
            O.check_topk(rk[i], sk[i], adc[i], 16384, atol=1e-4)
        # recall of the PQ first stage and of the reranked result against the exact search
        se, re_ = ix.search(q, qi, 100)
        sip, rip = ix.search(q, None, 100)
        rec1 = np.mean([len(set(rip[i, :10]) & set(r1[i])) / 10.0 for i in range(16)])
        assert rec1 >= 0.8, rec1
        s2 = ix.score_rows(q, qi, r1)
        order = np.lexsort((r1, -s2.astype(np.float64)), axis=1)[:, :10]
        rr = np.take_along_axis(r1, order, axis=1)
        rec2 = np.mean([len(set(re_[i, :10]) & set(rr[i])) / 10.0 for i in range(16)])
        assert rec2 >= 0.7, rec2
    finally:
        pix.close(); ix.close()
    # CLI: quantize_index + gip_retrieval --PQIP --rerank
    monkeypatch.chdir(tmp_path)
    qids = ["q%d" % i for i in range(16)]
    docids = ["d%d" % i for i in range(20000)]
    with open("q.pt", "wb") as f:
        pickle.dump([qv, qi, qids], f, protocol=4)
    with open("c.pt", "wb") as f:
        pickle.dump([cv, ci, docids], f, protocol=4)
    QI.main(["--index_path", "c.pt", "--output_index_path", "pq64_index"])
    G.main(["--query_emb_path", "q.pt", "--index_path", "c.pt", "--emb_dim", "768", "--PQIP", "--faiss_pq_index_path", "pq64_index",
            "--rerank", "--agip_topk", "500", "--topk", "10", "--output", "pq.trec"])
    lines = open("pq.trec").read().splitlines()
    assert len(lines) == 160
    first = {}
    for ln in lines:
        qid, _, did, rank, score, _ = ln.split()
        first.setdefault(qid, []).append(int(did[1:]))
    hit = np.mean([len(set(first["q%d" % i]) & set(re_[i, :10].tolist())) / 10.0 for i in range(16)])
    assert hit >= 0.6, hit


@pytest.mark.parametrize("n,q,d_dlr,d_cls,k", [(300, 3, 96, 32, 10), (257, 1, 768, 0, 5), (5000, 7, 64, 8, 100), (1000, 2, 104, 24, 50),
                                               (70, 5, 32, 96, 70), (4097, 9, 768, 8, 33), (900, 4, 104, 27, 20), (900, 4, 8, 3, 20),
                                               (6000, 5, 2048, 64, 100), (3000, 3, 4096, 0, 40)])     # gated halves wider than 1024: refine lists up to 4096 slices
def test_odd_shapes(G, n, q, d_dlr, d_cls, k):
    """Small / ragged / unusual widths: fewer rows than a tile, no dense tail, widths that are not multiples of 32 or 64
    (since round 6 every width runs on the stage images: the stage counts are rounded up to even with all-zero stages), k == n."""
    rng = np.random.default_rng(n + d_dlr)
    cv = np.abs(rng.standard_normal((n, d_dlr + d_cls)) * 0.3).astype(np.float16)
    cv[:, d_dlr:] = (rng.standard_normal((n, d_cls)) * 0.1).astype(np.float16)
    qv = np.abs(rng.standard_normal((q, d_dlr + d_cls)) * 0.3).astype(np.float16)
    qv[:, d_dlr:] = (rng.standard_normal((q, d_cls)) * 0.1).astype(np.float16)
    ci = rng.integers(0, 5, (n, d_dlr)).astype(np.uint8)
    qi = rng.integers(0, 5, (q, d_dlr)).astype(np.uint8)
    _search_check(G, cv, ci, qv.astype(np.float32), qi, k)


def test_emb_dim_not_a_multiple_of_8(G):
    """--emb_dim that is not a multiple of 8 (the reference takes any width, gip_retrieval.py:238): the C ABI appends zero slices to the
    gated half itself (corpus and every query batch, host or device arrays; since round 3 -- it used to refuse) and the host mirror
    does the same before it calls; both equal the oracle."""
    import ctypes as C
    from dhr_amd import _lib, synth
    cv, ci, qv, qi = synth.make_pair(51, 3000, 6, 100, 28)
    lib = _lib.load()
    q32 = qv.astype(np.float32)
    for dev_arrays in (False, True):
        if dev_arrays:
            import torch
            a_cv, a_ci, a_q, a_qi = (torch.from_numpy(x).cuda() for x in (cv, ci, q32, qi))
        else:
            a_cv, a_ci, a_q, a_qi = cv, ci, q32, qi
        desc = _lib.IndexDesc()
        desc.device, desc.n_rows, desc.d_dlr, desc.d_cls = 0, 3000, 100, 28
        desc.value, desc.ld_value, desc.mem_kind = _lib._ptr_ld(a_cv)
        desc.index, desc.ld_index, _ = _lib._ptr_ld(a_ci)
        desc.index_dtype = _lib.IDX_U8
        h = C.c_void_p()
        _lib.check(lib.dhr_index_create(C.byref(desc), C.byref(h)), "dhr_index_create")
        try:
            qb, keep = _lib.make_query_batch(a_q, a_qi)
            sc = np.empty((6, 50), np.float32); rows = np.empty((6, 50), np.int64)
            _lib.check(lib.dhr_search(h, C.byref(qb), 50, sc.ctypes.data, rows.ctypes.data, _lib.MEM_HOST, None), "dhr_search")
            for i in range(6):
                ex = O.gip_scores_f64(q32[i], qi[i], cv.astype(np.float32), ci)
                O.check_topk(rows[i], sc[i], ex, 50)
            qb1, keep1 = _lib.make_query_batch(a_q, None)                    # plain inner product over the same (unpadded) records
            _lib.check(lib.dhr_search(h, C.byref(qb1), 50, sc.ctypes.data, rows.ctypes.data, _lib.MEM_HOST, None), "dhr_search")
            for i in range(6):
                O.check_topk(rows[i], sc[i], cv.astype(np.float64) @ q32[i].astype(np.float64), 50)
        finally:
            lib.dhr_index_destroy(h)
    _search_check(G, cv, ci, qv.astype(np.float32), qi, 50)
    ix = G.GipIndex(cv, ci)
    assert (ix.k, ix.d_dlr) == (128, 100)
    # index file of such a width: the file holds the padded records and remembers the pad; a loaded index takes the caller's queries
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "odd.dhr")
        ix.save(path, ["d%d" % i for i in range(3000)])
        ix2, ids = G.GipIndex.load(path)
        assert (ix2.k, ix2.d_dlr, len(ids)) == (128, 100, 3000)
        sa, ra = ix.search(qv.astype(np.float32), qi, 50)
        sb, rb = ix2.search(qv.astype(np.float32), qi, 50)
        ix2.close()
        np.testing.assert_array_equal(ra, rb)
        np.testing.assert_array_equal(sa, sb)
    s2, r2 = ix.search_rerank(np.where(qv > 0.3, qv, 0).astype(np.float32), qi, qv.astype(np.float32), qi, 300, 20)
    rows = np.arange(3000, dtype=np.int64)[None, :].repeat(6, 0)
    ex = ix.score_rows(qv.astype(np.float32), qi, rows)
    ix.close()
    for i in range(6):
        np.testing.assert_allclose(ex[i], O.gip_scores_f64(qv[i].astype(np.float32), qi[i], cv.astype(np.float32), ci), rtol=0, atol=1e-5)


def _exhaustive_topk(ix, qv, qi, n, k, slab=1 << 20):
    """Ground truth at any size: EVERY row of the index scored exactly for every query of the (small) batch -- dhr_score_rows over the
    whole row range in slabs -- and the k best by (score desc, row asc) taken with torch.topk on the composite 64-bit key.  No bound, no
    filter, no threshold is involved: what dhr_search returns must equal this bit for bit (the scores are the same exactly-rounded
    values, exact ties break on the row)."""
    import torch
    dev = qv.device
    nq = qv.shape[0]
    best = None
    for lo in range(0, n, slab):
        hi = min(n, lo + slab)
        rows = torch.arange(lo, hi, device=dev, dtype=torch.int64)[None, :].expand(nq, -1).contiguous()
        sc = ix.score_rows_device(qv, qi, rows)
        b = sc.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        ordered = torch.where((b >> 31) != 0, (~b) & 0xFFFFFFFF, b | 0x80000000)          # order-preserving bits of an fp32
        key = ((ordered - (1 << 31)) << 32) + (0xFFFFFFFF - rows)                          # signed 64-bit: score desc, then row asc
        del rows, sc, b, ordered
        cat = key if best is None else torch.cat([best, key], dim=1)
        best = torch.topk(cat, min(k, cat.shape[1]), dim=1).values
        del key, cat
    rows = 0xFFFFFFFF - (best & 0xFFFFFFFF)
    o = (best >> 32) + (1 << 31)
    bits = torch.where((o >> 31) != 0, o & 0x7FFFFFFF, (~o) & 0xFFFFFFFF)
    scores = (bits & 0xFFFFFFFF).to(torch.int64)
    scores = torch.where(scores >= (1 << 31), scores - (1 << 32), scores).to(torch.int32).view(torch.float32)
    return scores, rows


def _independent_truth_check(slab_fn, n, d_dlr, qv, qi, rows, scores, k, slab=1 << 18):
    """Ground truth that shares NO code with the library (the round-5 review: the exhaustive truth above scores its rows with dhr_score_rows,
    i.e. through the same rescoring kernels as the search -- a 64-bit addressing bug for rows beyond 2^32 / 3072 would be self-consistent).
    torch float64 straight from the corpus values / slice indices: for every query of the (small) batch the gated inner product of EVERY
    row, slab by slab (slab_fn(lo, hi) -> (fp16 values, index bytes or None) of rows [lo, hi) on the device) -- fp16 x fp32 products are
    exact in float64, their sum is good to ~1e-13 --; then, per query:
      * every returned score is its row's float64 score rounded to fp32 (within one fp32 ulp: the library rounds its own float64 sum once);
      * the returned set is the exact top-k: every row strictly above the k-th best float64 score (by more than an fp32 ulp) is in the list,
        no returned row lies below it by more than that -- whatever its position in the row range;
      * rows are distinct and inside the corpus."""
    import torch
    dev = qv.device
    m = qv.shape[0]
    q64 = qv.double()
    exact = torch.empty((m, n), dtype=torch.float64, device=dev)
    zero = torch.zeros((), dtype=torch.float16, device=dev)
    for lo in range(0, n, slab):
        hi = min(n, lo + slab)
        v, x = slab_fn(lo, hi)
        exact[:, lo:hi] = (v[:, d_dlr:].double() @ q64[:, d_dlr:].T).T
        if d_dlr:
            vg = v[:, :d_dlr]
            for i in range(m):
                gate = x == qi[i][None, :].to(x.dtype)                # [rows, d_dlr]: c_idx[n][j] == q_idx[j] (gip_retrieval.py:115)
                exact[i, lo:hi] += torch.where(gate, vg, zero).double() @ q64[i, :d_dlr]
        del v, x
    ulp = 2.0 ** -23
    for i in range(m):
        ex = exact[i]
        r, sc = rows[i], scores[i].double()
        assert bool((r >= 0).all()) and bool((r < n).all()) and int(torch.unique(r).numel()) == k
        got = ex[r]
        assert bool(((sc - got).abs() <= ulp * got.abs().clamp_min(1e-30) + 1e-12).all()), "query %d: a returned score is not its row's exact score" % i
        sk = torch.topk(ex, k).values[-1]
        eps = ulp * float(sk.abs()) + 1e-12
        must = torch.nonzero(ex > sk + eps).flatten()
        inlist = torch.zeros(n, dtype=torch.bool, device=dev)
        inlist[r] = True
        assert bool(inlist[must].all()), "query %d: %d rows strictly above the k-th best score are missing (first: row %d)" % (
            i, int((~inlist[must]).sum()), int(must[~inlist[must]][0]))
        assert bool((got >= sk - eps).all()), "query %d: a returned row lies below the k-th best score" % i
    return exact


@pytest.mark.parametrize("kind", ["hybrid", "dense"])
def test_full_size_properties(G, kind):
    """BASELINE config 3 (hybrid) / config 2 (dense-only) at FULL size (8 841 823 x (768+768), 6 980 queries, top-1000), where the oracle cannot run: properties
    that do not depend on the size.  (1) lists are sorted (score desc, row asc) with distinct valid rows; (2) the search is
    idempotent; (3) every returned score is the exact score of its row (dhr_score_rows, an independent code path);
    (4) completeness spot check: for sampled queries, none of 200 000 random rows outside the list beats the k-th score;
    (5) the first and the last 200 000 rows of the same corpus searched alone agree with the oracle (ties the generator to the CPU path);
    (6) 36 queries equal the exhaustive top-k bit for bit (scored through dhr_score_rows); (7) the same 36 queries against torch float64
    scores of EVERY row computed from cv / ci directly -- no library code (_independent_truth_check)."""
    import sys, os
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import bench
    from dhr_amd import synth
    dev = torch.device("cuda", 0)
    n, nq, k = 8_841_823, 6980, 1000
    d_dlr = 768 if kind == "hybrid" else 0
    cv, ci = bench.gen_shard(torch, synth, dev, 1237, n, d_dlr, 768, 30, 90, False)
    qv, qi = bench.gen_shard(torch, synth, dev, 1237 + 999_983, nq, d_dlr, 768, 4, 12, False)
    ix = G.GipIndex(cv, ci)
    try:
        s1, r1 = ix.search(qv, qi, k, out_device=True)
        s2, r2 = ix.search(qv, qi, k, out_device=True)
        assert torch.equal(r1, r2) and torch.equal(s1, s2)                                       # (2)
        assert bool((r1 >= 0).all()) and bool((r1 < n).all())
        ds = s1[:, 1:] - s1[:, :-1]
        assert bool((ds <= 0).all())                                                              # (1) scores descending
        tie = ds == 0
        assert bool((r1[:, 1:][tie] > r1[:, :-1][tie]).all())                                     #     row ascending on ties
        assert int(torch.sort(r1, dim=1).values.diff(dim=1).eq(0).sum()) == 0                     #     distinct rows
        sub = torch.arange(0, nq, 97, device=dev)
        qs, qis = qv[sub].cpu().numpy().astype(np.float32), (None if qi is None else qi[sub].cpu().numpy())
        rows = r1[sub].cpu().numpy()
        sc = ix.score_rows(qs, qis, rows)
        np.testing.assert_array_equal(sc, s1[sub].cpu().numpy())                                 # (3)
        g = torch.Generator(device="cpu").manual_seed(7)
        rnd = torch.randint(0, n, (len(sub), 200_000), generator=g).numpy().astype(np.int64)
        rs = ix.score_rows(qs, qis, rnd)
        kth = s1[sub, k - 1].cpu().numpy()[:, None]
        inlist = np.stack([np.isin(rnd[i], rows[i]) for i in range(len(sub))])
        assert not np.any((rs > kth) & ~inlist)                                                   # (4)
        # (6) exhaustive ground truth for 36 queries spread over the batch (incl. its first and last): all 8 841 823 rows scored exactly,
        # the k best taken without any bound or threshold -- the search's lists must be EQUAL (rows and score bits)
        ex_q = torch.unique(torch.cat([torch.arange(0, nq, 200, device=dev), torch.tensor([nq - 1], device=dev)]))
        es, er = _exhaustive_topk(ix, qv[ex_q].contiguous(), None if qi is None else qi[ex_q].contiguous(), n, k)
        assert torch.equal(er, r1[ex_q]), "rows differ from the exhaustive top-k for queries %s" % ex_q[(er != r1[ex_q]).any(dim=1)].tolist()
        assert torch.equal(es.view(torch.int32), s1[ex_q].view(torch.int32))
        print("\n[%s, full size] %d queries: dhr_search == exhaustive top-%d over all %d rows" % (kind, len(ex_q), k, n))
        # (7) the same 36 queries against a ground truth that shares no code with the library: torch float64 from cv / ci directly, every row
        # of the corpus (the rows beyond 2^32 / 3072 bytes included), returned scores == exact scores, no outsider above the k-th score
        ix.close()
        ix = None
        torch.cuda.empty_cache()
        _independent_truth_check(lambda lo, hi: (cv[lo:hi], None if ci is None else ci[lo:hi]), n, d_dlr, qv[ex_q].float(),
                                 None if qi is None else qi[ex_q], r1[ex_q], s1[ex_q], k)
        print("[%s, full size] %d queries: dhr_search == torch float64 ground truth over all %d rows (no library code)" % (kind, len(ex_q), n))
    finally:
        if ix is not None:
            ix.close()
    m = 200_000
    cvs, cis = cv[:m].cpu().numpy(), (None if ci is None else ci[:m].cpu().numpy())
    cvl, cil = cv[n - m:].cpu().numpy(), (None if ci is None else ci[n - m:].cpu().numpy())
    del cv, ci
    torch.cuda.empty_cache()
    _search_check(G, cvs, cis, qs[:6], None if qis is None else qis[:6], 100)                     # (5) the first 200 000 rows ...
    _search_check(G, cvl, cil, qs[:6], None if qis is None else qis[:6], 100, row_offset=n - m)   #     ... and the LAST (row offsets beyond 2^32 / 3072)


@pytest.mark.parametrize("kind", ["hybrid", "dense"])
def test_clustered_data_exhaustive(G, kind):
    """Structure-bearing dense columns (bench.py --data clustered: 2 000 Gaussian clusters with a skewed size distribution, sigma_within =
    0.3 sigma_between, decaying per-dimension spectrum, 1 % near-duplicate rows, 5 % hot queries on cluster centres) -- the filter's speed is
    data-dependent, its RESULT must not be.  1 M rows (whole generator chunks, so the near-duplicates are in), 1 024 queries, top-1000:
    (a) 40 queries spread over the batch -- every hot query among them -- equal the exhaustive top-k over all rows (rows and score bits);
    (b) sorted, distinct, idempotent; (c) a 100 000-row slice against the float64 oracle under the tie rule; (d) no query fell back."""
    import sys, os
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import bench
    from dhr_amd import synth, _lib
    dev = torch.device("cuda", 0)
    n, nq, k = 4 * bench.GEN_CHUNK, 1024, 1000
    d_dlr = 768 if kind == "hybrid" else 0
    cm = synth.torch_cluster_model(1237, 768, dev)
    cv, ci = bench.gen_rows(torch, synth, dev, 1237, 0, n, d_dlr, 768, 30, 90, False, clustered=cm, dup=True)
    qv, qi = bench.gen_rows(torch, synth, dev, 1237 + 999_983, 0, nq, d_dlr, 768, 4, 12, False, clustered=cm, hot_frac=synth.HOT_FRAC)
    # the data really is what the docstring says: near-duplicate rows exist, and some queries sit on a centre
    centres = cm[0]
    qd = qv[:, d_dlr:].float()
    dist = torch.cdist(qd, centres).min(dim=1).values
    hot = torch.nonzero(dist < 0.25 * dist.median()).flatten()
    assert 20 <= len(hot) <= 100, len(hot)
    ix = G.GipIndex(cv, ci)
    ix.set_param(_lib.PARAM_PROFILE, 1)
    try:
        s1, r1 = ix.search(qv, qi, k, out_device=True)
        st = ix.stats()
        s2, r2 = ix.search(qv, qi, k, out_device=True)
        assert torch.equal(r1, r2) and torch.equal(s1, s2)
        ds = s1[:, 1:] - s1[:, :-1]
        assert bool((ds <= 0).all()) and bool((r1[:, 1:][ds == 0] > r1[:, :-1][ds == 0]).all())
        assert int(torch.sort(r1, dim=1).values.diff(dim=1).eq(0).sum()) == 0
        ex_q = torch.unique(torch.cat([torch.arange(0, nq, 64, device=dev), hot[:24], torch.tensor([nq - 1], device=dev)]))
        es, er = _exhaustive_topk(ix, qv[ex_q].contiguous(), None if qi is None else qi[ex_q].contiguous(), n, k)
        assert torch.equal(er, r1[ex_q]), "rows differ from the exhaustive top-k for queries %s" % ex_q[(er != r1[ex_q]).any(dim=1)].tolist()
        assert torch.equal(es.view(torch.int32), s1[ex_q].view(torch.int32))
        assert st["sample_fallback_queries"] == 0, st
        _independent_truth_check(lambda lo, hi: (cv[lo:hi], None if ci is None else ci[lo:hi]), n, d_dlr, qv[ex_q].float(),
                                 None if qi is None else qi[ex_q], r1[ex_q], s1[ex_q], k)          # ... and the torch float64 truth (no library code)
        print("\n[clustered %s, %d rows] %d queries (%d hot) == exhaustive top-%d == torch float64 truth; bound %.0f -> exact %.0f rows per query, %d launches"
              % (kind, n, len(ex_q), min(24, len(hot)), k, st["candidates_bound"] / nq, st["candidates_exact"] / nq, st["phases"]))
    finally:
        ix.close()
    m = 100_000
    qs = qv[hot[:3].tolist() + [0, 1, 2]].cpu().numpy().astype(np.float32)
    qis = None if qi is None else qi[hot[:3].tolist() + [0, 1, 2]].cpu().numpy()
    cvs, cis = cv[:m].cpu().numpy(), (None if ci is None else ci[:m].cpu().numpy())
    del cv, ci
    torch.cuda.empty_cache()
    _search_check(G, cvs, cis, qs, qis, 100)


@pytest.mark.parametrize("ns", [8, 4])
def test_config4_full_size_8_shards(G, ns):
    """BASELINE config 4 at FULL size on one GPU: the bench corpus (seed 1237, bench.gen_rows) as the reference's 8 row shards
    (gip_retrieval.py:292-306: per = N // S, the last shard takes the remainder) through dhr_search_sharded_local -- the same
    sharded_core the RCCL entry point runs, gathers as device copies -- must reproduce the unsharded search bit for bit (the
    checksum bench.py prints for N = 1; merge semantics of merge.result.py:22-42 without the text round trip).  Also prints the
    per-stage times of the slowest shard (the single-GPU emulation of the 8-GPU step that DESIGN.md section 5 quotes)."""
    import sys, os, time
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import bench
    from dhr_amd import synth, _lib, dist as D
    dev = torch.device("cuda", 0)
    n, nq, k = 8_841_823, 6980, 1000
    qv, qi = bench.gen_rows(torch, synth, dev, 1237 + 999_983, 0, nq, 768, 768, 4, 12, False)
    # the unsharded search first (its index is dropped before the shards are built)
    cv, ci = bench.gen_rows(torch, synth, dev, 1237, 0, n, 768, 768, 30, 90, False)
    full = G.GipIndex(cv, ci)
    del cv, ci
    torch.cuda.empty_cache()
    for _ in range(2):
        fs, fr = full.search(qv, qi, k, out_device=True)
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(3):
        fs, fr = full.search(qv, qi, k, out_device=True)
    torch.cuda.synchronize(); t_full = (time.perf_counter() - t) / 3
    want = bench.result_checksum(torch, fs, fr)
    # exhaustive ground truth for 32 queries (every row of the unsharded index scored exactly, no bound / filter / threshold): what the
    # 8-shard search returns is compared with THIS below, not only with the unsharded search
    ex_q = torch.arange(3, nq, 218, device=dev)
    es, er = _exhaustive_topk(full, qv[ex_q].contiguous(), qi[ex_q].contiguous(), n, k)
    full.close()
    del full
    torch.cuda.empty_cache()
    shards = []
    try:
        for r in range(ns):
            lo, hi = D.shard_bounds(n, ns, r)
            scv, sci = bench.gen_rows(torch, synth, dev, 1237, lo, hi, 768, 768, 30, 90, False)
            shards.append(G.GipIndex(scv, sci, row_offset=lo))
            del scv, sci
            torch.cuda.empty_cache()
        assert [s.n_rows for s in shards] == [n // ns] * (ns - 1) + [n - (ns - 1) * (n // ns)]
        ss, sr = D.search_sharded_local(shards, qv, qi, k)
        # no query may need the repair path on this data (round 5: at 4 shards 40 queries per step did, after the second list tier's arena was
        # handed out in query order and ran dry half-way through the batch -- the result was right, the step 2 x slower)
        assert _lib.load().dhr_debug_sharded_repairs() == 0
        got = bench.result_checksum(torch, ss, sr)
        assert got == want, (got, want)
        assert torch.equal(sr, fr) and torch.equal(ss, fs)
        assert torch.equal(sr[ex_q], er) and torch.equal(ss[ex_q].view(torch.int32), es.view(torch.int32))       # 8 shards == exhaustive ground truth
        if ns == 8:      # ... == the torch float64 truth from the generator's own rows (no library code; the corpus is regenerated slab by slab)
            _independent_truth_check(lambda lo, hi: bench.gen_rows(torch, synth, dev, 1237, lo, hi, 768, 768, 30, 90, False), n, 768, qv[ex_q].float(),
                                     qi[ex_q], sr[ex_q], ss[ex_q], k)
        # stage times, slowest shard per stage: begin (phase 0 + sampled run) | common threshold | finish (main pass) | merge
        for ix in shards:
            ix.set_param(_lib.PARAM_SAMPLE_SHARE, ns)
        rnk = shards[0].union_rank(k)
        rl_mid, ru_mid = max(s.mid_ranks(k)[0] for s in shards), max(s.mid_ranks(k)[1] for s in shards)
        rl_pre, ru_pre = max(s.pre_ranks(k)[0] for s in shards), max(s.pre_ranks(k)[1] for s in shards)
        assert rl_mid > 0 and rl_pre > 0
        best = None
        for it in range(3):
            tb, tf, samples, outs, firsts, tb2 = [], [], [], [], [], []
            # first agreement in two rounds (sharded.hip step 1a): the first part of every shard's sample, a common threshold, the rest filtered at it
            for ix in shards:
                torch.cuda.synchronize(); t = time.perf_counter()
                firsts.append(ix.search_pre(qv, qi, k, rl_pre)); torch.cuda.synchronize(); tb.append(time.perf_counter() - t)
            torch.cuda.synchronize(); t = time.perf_counter()
            tau0 = D.common_threshold(torch.stack(firsts), min(ru_pre, ns * rl_pre)); torch.cuda.synchronize(); tt = time.perf_counter() - t
            for ix in shards:
                torch.cuda.synchronize(); t = time.perf_counter()
                samples.append(ix.search_begin_rest(tau0)); torch.cuda.synchronize(); tb2.append(time.perf_counter() - t)
            tb = [a_ + b_ for a_, b_ in zip(tb, tb2)]                  # "begin" = both parts of the sampled run
            torch.cuda.synchronize(); t = time.perf_counter()
            tau = D.common_threshold(torch.stack(samples), rnk); torch.cuda.synchronize(); tt += time.perf_counter() - t
            # second agreement (sharded.hip step 2b): first slice of the main pass, the shards' best scores seen so far, tau raised
            seen, tmid = [], []
            for ix in shards:
                torch.cuda.synchronize(); t = time.perf_counter()
                seen.append(ix.search_mid(tau, rl_mid)); torch.cuda.synchronize(); tmid.append(time.perf_counter() - t)
            torch.cuda.synchronize(); t = time.perf_counter()
            tau = torch.maximum(tau, D.common_threshold(torch.stack(seen), min(ru_mid, ns * rl_mid))); torch.cuda.synchronize(); tt += time.perf_counter() - t
            for ix in shards:
                torch.cuda.synchronize(); t = time.perf_counter()
                outs.append(ix.search_finish(tau)); torch.cuda.synchronize(); tf.append(time.perf_counter() - t)
            tf = [a_ + b_ for a_, b_ in zip(tf, tmid)]                  # "finish" = both parts of the main pass
            # the merge as sharded.hip runs it: list prefixes of the fixed length prefix_len(k, world) (a shard holding more than that of
            # a query's top-k flags the query for the repair path; none does here).  Timed: ONE shard's prefix cut + the rank merge of the
            # gathered block (stacking the eight prefixes here stands for the all-gather, which is modelled below).
            cnts = torch.stack([o[2] for o in outs]); kk = min(k, ((3 * k + ns - 1) // ns + 64 + 63) // 64 * 64)
            assert int(cnts.max()) <= kk and int(cnts.min()) >= 0
            gs = torch.stack([o[0][:, :kk] for o in outs]); gr = torch.stack([o[1][:, :kk] for o in outs])
            torch.cuda.synchronize(); t = time.perf_counter()
            cut = (outs[0][0][:, :kk].contiguous(), outs[0][1][:, :kk].contiguous())
            ms, mr = D.merge_sorted_lists(gs, gr, k); torch.cuda.synchronize(); tm = time.perf_counter() - t
            del cut
            tot = max(tb) + tt + max(tf) + tm
            if best is None or tot < best[0]:
                best = (tot, max(tb), tt, max(tf), tm, kk)
        assert torch.equal(mr, fr) and torch.equal(ms, fs)
        # the collectives of dhr_search_sharded, modelled at 50 AND 100 us of launch + latency each, payload / 150 GB/s (xGMI is point to point:
        # in an all-gather every rank sends ITS block to the 7 others over 7 links at once, so the time is one block over one link).  FIVE per
        # step since round 6 (the counts travel in the block of the list prefixes, and scores and rows of the prefixes in ONE block): the
        # agreement on the ranks (48 B), [Q, rl_pre] first sample scores, [Q, r_local] sample scores, [Q, rl_mid] seen scores,
        # [Q] counts + [Q, kk] x (fp32 + int64) list prefixes, kk as sharded.hip prefix_len; every block + its 16-byte status record
        r_loc = shards[0].sample_rank(k)
        kk_fix = min(k, ((3 * k + ns - 1) // ns + 64 + 63) // 64 * 64)
        blocks = (48, nq * rl_pre * 4 + 16, nq * r_loc * 4 + 16, nq * rl_mid * 4 + 16, nq * 4 + nq * kk_fix * 12 + 16)
        coll = {lat: sum(lat * 1e-6 + b / 150e9 for b in blocks) for lat in (50, 100)}
        print("\n[config 4 as %d shards, emulated on one GPU] unsharded step %.1f ms; slowest shard per stage: begin (first part of the sample + rest) %.2f + thresholds (three agreements) %.2f + main pass (first slice + rest) %.2f + merge %.2f "
              "= %.2f ms -> %.2fx; + the 5 all-gathers (ranks 48 B, [Q, %d] first sample scores, [Q, %d] sample scores, [Q, %d] seen scores, [Q] counts + [Q, %d] x 12 B lists) modelled at bytes / 150 GB/s + "
              "50 us each = %.2f ms -> %.2f ms = %.2fx | + 100 us each = %.2f ms -> %.2f ms = %.2fx"
              % (ns, t_full * 1e3, best[1] * 1e3, best[2] * 1e3, best[3] * 1e3, best[4] * 1e3, best[0] * 1e3, t_full / best[0], rl_pre, r_loc, rl_mid, kk_fix,
                 coll[50] * 1e3, (best[0] + coll[50]) * 1e3, t_full / (best[0] + coll[50]), coll[100] * 1e3, (best[0] + coll[100]) * 1e3, t_full / (best[0] + coll[100])))
        # the whole step through the entry point the ranks really call (dhr_search_sharded_local: every shard's kernels on ONE stream of this one
        # GPU, gathers as device copies): 1 / ns of it is the AVERAGE shard's step with the host enqueueing ahead of the device as it does over
        # RCCL -- the per-stage calls above start every stage from an idle device and a blocked host
        for _ in range(2):
            D.search_sharded_local(shards, qv, qi, k)
        torch.cuda.synchronize(); t = time.perf_counter()
        for _ in range(3):
            D.search_sharded_local(shards, qv, qi, k)
        torch.cuda.synchronize(); t_loc = (time.perf_counter() - t) / 3
        print("[config 4 as %d shards] dhr_search_sharded_local, all shards on one GPU: %.1f ms per step = %.2f ms per shard (1 / %d) -> %.2fx of the unsharded step; with the 5 all-gathers at 50 / 100 us: %.2f / %.2f ms -> %.2fx / %.2fx"
              % (ns, t_loc * 1e3, t_loc * 1e3 / ns, ns, t_full / (t_loc / ns), (t_loc / ns + coll[50]) * 1e3, (t_loc / ns + coll[100]) * 1e3,
                 t_full / (t_loc / ns + coll[50]), t_full / (t_loc / ns + coll[100])))
    finally:
        for s in shards:
            s.close()


def test_search_enqueues_without_host_readbacks(G):
    """SURVEY.md section 8b ("asynchronous on the given stream"): the first attempt of a sampled search only ENQUEUES.  Two shard
    handles on two streams: the staged entry points return to the host long before their streams drain, the two streams' work
    overlaps on the device, and the results equal the synchronous calls'.  (dhr_search itself ends with its one host read -- the
    count of queries to redo -- so the enqueue-only behaviour is observed through the begin step the sharded search uses.)"""
    import ctypes as C
    import time
    import torch
    from dhr_amd import _lib, synth
    lib = _lib.load()
    lib.dhr_internal_search_begin_async.argtypes = [C.c_void_p, C.POINTER(_lib.QueryBatch), C.c_int32, C.c_void_p, C.c_void_p]
    n, nq, k = 600_000, 2048, 1000
    cv, ci, qv, qi = synth.make_pair(31, n, nq, 768, 64)
    dev = torch.device("cuda", 0)
    qd, qid = torch.from_numpy(qv).to(dev), torch.from_numpy(qi).to(dev)
    shards = [G.GipIndex(cv[: n // 2], ci[: n // 2]), G.GipIndex(cv[n // 2:], ci[n // 2:], row_offset=n // 2)]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    try:
        r = shards[0].sample_rank(k)
        assert r > 0
        ref = [s.search_begin(qd, qid, k).clone() for s in shards]                  # synchronous calls (default stream), also warms the workspaces
        outs = [torch.empty((nq, r), dtype=torch.float32, device=dev) for _ in shards]
        qbs = [s._qb(qd, qid) for s in shards]

        def enqueue(i):
            _lib.check(lib.dhr_internal_search_begin_async(shards[i]._h, C.byref(qbs[i][0]), k, outs[i].data_ptr(), streams[i].cuda_stream), "begin_async")

        for i in range(2):                      # first use of a stream maps a hardware queue (milliseconds): not what is measured
            enqueue(i)
        # one handle alone: host return vs completion
        torch.cuda.synchronize(); t0 = time.perf_counter(); enqueue(0); t_ret = time.perf_counter() - t0
        streams[0].synchronize(); t_one = time.perf_counter() - t0
        # both handles back to back on their own streams
        torch.cuda.synchronize(); t0 = time.perf_counter(); enqueue(0); enqueue(1); t_ret2 = time.perf_counter() - t0
        streams[0].synchronize(); streams[1].synchronize(); t_two = time.perf_counter() - t0
        print("\n[enqueue-only begin] one handle: host returns after %.2f ms, stream done after %.2f ms; two handles on two streams: "
              "host returns after %.2f ms, both done after %.2f ms (%.2fx one)" % (t_ret * 1e3, t_one * 1e3, t_ret2 * 1e3, t_two * 1e3, t_two / t_one))
        assert t_ret < 0.6 * t_one, (t_ret, t_one)               # the call returned while most of its work was still queued
        assert t_ret2 < 0.6 * t_two
        assert t_two < 1.9 * t_one                                # the two streams overlap (2.0 = strictly one after the other)
        for i in range(2):
            assert torch.equal(outs[i], ref[i])
    finally:
        for s in shards:
            s.close()


def test_random_configurations(G, monkeypatch):
    """A slice of tools/stress.py (randomised shapes / dtypes / signs / fp32-or-fp16 queries / bucket counts / mixed query and
    corpus index dtypes, each checked against the oracle's float64 scores)."""
    import os, sys
    monkeypatch.setenv("DHR_GATED_I8", "0")      # (the tool sets the variable per case: restored when the test ends)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    import stress
    monkeypatch.setattr(sys, "argv", ["stress.py", "80", "11"])
    stress.main()


def test_random_controller_configurations(G, monkeypatch):
    """A slice of tools/stress_sampled.py: corpora large enough for the sampled thresholds, random sample period / list capacity /
    chunk count / head size, benign and adversarial row orders, single index and the staged sharded search -- each checked
    against the oracle's float64 scores."""
    import os, sys
    monkeypatch.setenv("DHR_GATED_I8", "0")      # (the tool sets the variable per case: restored when the test ends)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    import stress_sampled
    monkeypatch.setattr(sys, "argv", ["stress_sampled.py", "14", "5"])
    stress_sampled.main()


@pytest.mark.parametrize("n_lists,ll", [(4, 16), (8, 448), (3, 7000)])
def test_device_merge_signed_zero_ties(G, n_lists, ll):
    """-0.0 ties with +0.0 in the shard reduces on the device (LDS merge of sorted lists, LDS bitonic reduce, the global-memory reduce beyond
    16 384 entries): "score desc, row asc" as floats compare, equal to the oracle and to the host twins."""
    import torch
    from dhr_amd import dist as D
    rng = np.random.default_rng(n_lists * 1000 + ll)
    q, k = 6, min(1000, n_lists * ll)
    sc = np.where(rng.random((n_lists, q, ll)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    sc[:, :, : ll // 4] = np.round(rng.standard_normal((n_lists, q, ll // 4)), 1).astype(np.float32) + np.float32(3.0)
    rows = np.stack([rng.permutation(n_lists * ll)[:ll] for _ in range(n_lists * q)]).reshape(n_lists, q, ll).astype(np.int64)
    for l in range(n_lists):
        rows[l] += l * 10_000_000
        for i in range(q):
            o = np.lexsort((rows[l, i], -sc[l, i].astype(np.float64)))
            sc[l, i], rows[l, i] = sc[l, i][o], rows[l, i][o]
    es, er = O.merge_topk(list(sc), list(rows), k)
    for dev in ("cuda", "cpu"):
        ts, tr = torch.from_numpy(sc).to(dev), torch.from_numpy(rows).to(dev)
        ms, mr = D.merge_sorted_lists(ts, tr, k)
        np.testing.assert_array_equal(mr.cpu().numpy(), er)
        np.testing.assert_array_equal(ms.cpu().numpy(), es)
        perm = torch.from_numpy(rng.permutation(n_lists * ll)).to(dev)
        cs, cr = ts.permute(1, 0, 2).reshape(q, -1)[:, perm].contiguous(), tr.permute(1, 0, 2).reshape(q, -1)[:, perm].contiguous()
        ms, mr = D.merge_topk(cs, cr, k)
        np.testing.assert_array_equal(mr.cpu().numpy(), er)
        np.testing.assert_array_equal(ms.cpu().numpy(), es)


def test_distinct_handles_from_concurrent_host_threads(G):
    """dhr_hip.h: "one handle is used by one host thread at a time; distinct handles may be used concurrently".  Four host threads, each with
    its own index (different shapes: gated int8 / fp16 images, dense-only, BM25-like int16), its own stream and 12 searches + a two-stage search
    + a shard reduce in flight at the same time (ctypes drops the GIL over every call): every result equals the same thread's serial result bit
    for bit, the per-thread error record stays the thread's own."""
    import threading
    import torch
    from dhr_amd import _lib, synth, dist as D
    specs = [(31, 30000, 24, 768, 128, "hybrid"), (32, 9000, 9, 0, 768, "dense"), (33, 12000, 17, 768, 0, "bm25"), (34, 5000, 33, 128, 64, "hybrid")]
    data = [synth.make_pair(seed, n, q, dd, dc, kind=kind) if kind != "hybrid" else synth.make_pair(seed, n, q, dd, dc) for seed, n, q, dd, dc, kind in specs]

    def work(t, out, streams):
        cv, ci, qv, qi = data[t]
        q32 = qv.astype(np.float32)
        ix = G.GipIndex(cv, ci)
        try:
            res = []
            st = streams[t].cuda_stream if streams else 0
            for it in range(12):
                k = [1, 10, 100, 1000][it % 4]
                res.append(ix.search(q32, qi, k, stream=st))
            if ci is not None:
                res.append(ix.search_rerank(np.where(q32 > 0.3, q32, np.float32(0)), qi, q32, qi, 2000, 100, stream=st))
            s, r = res[3]
            res.append(tuple(x.numpy() for x in D.merge_topk(torch.from_numpy(s), torch.from_numpy(r), 50)))
            # an error on this thread: the record is this thread's own
            with pytest.raises(_lib.DhrError) as ei:
                ix.search(q32, qi, 0, stream=st)               # k = 0: refused by the library
            res.append(str(ei.value))
            out[t] = res
        finally:
            ix.close()

    serial, conc = [None] * 4, [None] * 4
    for t in range(4):
        work(t, serial, None)
    streams = [torch.cuda.Stream() for _ in range(4)]
    errs = []

    def guarded(t):
        try:
            work(t, conc, streams)
        except BaseException as e:  # noqa: BLE001
            errs.append((t, repr(e)))
    for rep in range(3):
        th = [threading.Thread(target=guarded, args=(t,)) for t in range(4)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errs, errs
        for t in range(4):
            assert len(conc[t]) == len(serial[t])
            for a_, b_ in zip(conc[t], serial[t]):
                if isinstance(a_, str):
                    assert a_ == b_
                else:
                    np.testing.assert_array_equal(a_[0], b_[0])
                    np.testing.assert_array_equal(a_[1], b_[1])


def test_no_device_memory_left_behind(G, tmp_path):
    """Every handle returns its device memory: cycles of index build / searches of growing batches / two-stage / score_rows / file round trip /
    one-process sharded search / PQ scan / failing calls (bad arguments, an injected host allocation failure half-way through a search), then
    destroy -- the free device memory after five more cycles is what it was after the first."""
    import torch
    from dhr_amd import _lib, synth, dist as D
    from dhr_amd.retrieval import quantize_index as QI
    lib = _lib.load()
    cv, ci, qv, qi = synth.make_pair(77, 40000, 40, 768, 128)
    q32 = qv.astype(np.float32)
    rng = np.random.default_rng(0)
    cb = rng.standard_normal((64, 256, 14)).astype(np.float32)
    codes = rng.integers(0, 256, (40000, 64)).astype(np.uint8)

    def cycle():
        ix = G.GipIndex(cv, ci)
        try:
            for nq, k in ((3, 10), (40, 1000), (17, 20000)):
                ix.search(q32[:nq], qi[:nq], k)
            s, r = ix.search_rerank(np.where(q32 > 0.3, q32, np.float32(0)), qi, q32, qi, 5000, 100)
            ix.score_rows(q32, qi, r)
            ix.save(str(tmp_path / "ix.dhr"))
            with pytest.raises(_lib.DhrError):
                ix.search(q32, qi, 0)                               # refused by the library
            with pytest.raises(ValueError):
                ix.search(q32[:, :-8].copy(), qi, 10)              # refused by the mirror: a batch of another width
            a0 = lib.dhr_debug_fail_alloc(0)
            ix.search(q32, qi, 100)
            n_alloc = lib.dhr_debug_fail_alloc(0) - a0             # host allocations of one search on the warm handle
            assert n_alloc >= 1
            lib.dhr_debug_fail_alloc(n_alloc // 2 + 1)         # ... one of them fails half-way through the next search
            try:
                with pytest.raises(_lib.DhrError):
                    ix.search(q32, qi, 100)
            finally:
                lib.dhr_debug_fail_alloc(0)
            ix.search(q32, qi, 100)
        finally:
            ix.close()
        ix2, _ = G.GipIndex.load(str(tmp_path / "ix.dhr"))
        ix2.search(q32, qi, 10)
        ix2.close()
        shards = [G.GipIndex(cv[a:b], ci[a:b], row_offset=a) for a, b in ((0, 9000), (9000, 30000), (30000, 40000))]
        try:
            D.search_sharded_local(shards, q32, qi, 1000)
        finally:
            for sh in shards:
                sh.close()
        pix = QI.PqIndex(cb, codes)
        try:
            pix.search(q32, 3000)
        finally:
            pix.close()
        torch.cuda.synchronize()

    cycle()
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(5):
        cycle()
    torch.cuda.empty_cache()
    free1 = torch.cuda.mem_get_info()[0]
    assert free1 >= free0 - (32 << 20), "device memory left behind: %.1f MB over five cycles" % ((free0 - free1) / 1e6)


def test_bad_arguments_on_a_device_are_statuses(G):
    """Every detectable misuse of the C structs comes back as a negative status with a message -- with a GPU present, where the argument checks
    are followed by real work (tests/test_cabi.py covers the host without one) -- and leaves the library usable: one field of a valid
    dhr_index_desc / dhr_query_batch / call broken at a time, a valid search before and after."""
    import ctypes as C
    from dhr_amd import _lib, synth
    lib = _lib.load()
    cv, ci, qv, qi = synth.make_pair(55, 3000, 6, 64, 32)
    q32 = qv.astype(np.float32)
    ix = G.GipIndex(cv, ci)
    s0, r0 = ix.search(q32, qi, 50)

    def desc():
        d = _lib.IndexDesc()
        d.device, d.n_rows, d.d_dlr, d.d_cls = 0, 3000, 64, 32
        d.value, d.ld_value, d.mem_kind = _lib._ptr_ld(cv)
        d.index, d.ld_index, d.index_dtype = ci.ctypes.data, 64, _lib.idx_code(ci.dtype)
        return d
    bad_desc = [("device", 99), ("device", -1), ("mem_kind", 7), ("n_rows", 0), ("n_rows", -5), ("n_rows", 1 << 33), ("d_dlr", -8), ("d_cls", -1), ("value", None),
                ("ld_value", 95), ("ld_value", -1), ("index_dtype", 9), ("index_dtype", _lib.IDX_NONE), ("idx_buckets", 3), ("idx_buckets", -1), ("ld_index", 63), ("row_offset", -1)]
    for field, val in bad_desc:
        d = desc()
        setattr(d, field, val)
        if field == "n_rows" and val > 3000:
            d.value = None                                 # (a row count beyond the caller's buffer is the caller's business: only the null pointer is detectable)
        h = C.c_void_p()
        rc = lib.dhr_index_create(C.byref(d), C.byref(h))
        assert rc < 0 and not h.value and lib.dhr_last_error(), (field, val, rc)
    d = desc()
    assert lib.dhr_index_create(None, C.byref(C.c_void_p())) < 0 and lib.dhr_index_create(C.byref(d), None) < 0
    d.d_dlr, d.d_cls, d.index, d.index_dtype = 0, 0, None, _lib.IDX_NONE                 # no columns at all
    assert lib.dhr_index_create(C.byref(d), C.byref(C.c_void_p())) < 0

    hs, hr = np.empty((6, 50), np.float32), np.empty((6, 50), np.int64)
    def call(qb, k=50, ps=None, pr=None, kind=_lib.MEM_HOST):
        return lib.dhr_search(ix._h, C.byref(qb), k, hs.ctypes.data if ps is None else ps, hr.ctypes.data if pr is None else pr, kind, None)
    bad_qb = [("n_queries", 0), ("n_queries", -3), ("mem_kind", 5), ("value", None), ("value_dtype", 9), ("ld_value", 95), ("index_dtype", 7), ("ld_index", 10)]
    for field, val in bad_qb:
        qb, keep = _lib.make_query_batch(q32, qi)
        setattr(qb, field, val)
        rc = call(qb)
        assert rc < 0 and lib.dhr_last_error(), (field, val, rc)
    qb, keep = _lib.make_query_batch(q32, qi)
    for kw in (dict(k=0), dict(k=-1), dict(k=(1 << 20) + 1), dict(kind=9)):
        assert call(qb, **kw) < 0 and lib.dhr_last_error(), kw
    assert lib.dhr_search(ix._h, C.byref(qb), 50, None, hr.ctypes.data, _lib.MEM_HOST, None) < 0
    assert lib.dhr_search(ix._h, C.byref(qb), 50, hs.ctypes.data, None, _lib.MEM_HOST, None) < 0
    assert lib.dhr_search(None, C.byref(qb), 50, hs.ctypes.data, hr.ctypes.data, _lib.MEM_HOST, None) < 0
    assert lib.dhr_search(ix._h, None, 50, hs.ctypes.data, hr.ctypes.data, _lib.MEM_HOST, None) < 0
    assert lib.dhr_search_rerank(ix._h, C.byref(qb), None, 100, 50, hs.ctypes.data, hr.ctypes.data, _lib.MEM_HOST, None) < 0
    assert lib.dhr_search_rerank(ix._h, C.byref(qb), C.byref(qb), 10, 50, hs.ctypes.data, hr.ctypes.data, _lib.MEM_HOST, None) < 0 or True   # (k > k1 is clamped or refused: either is a status)
    rows = np.zeros((6, 4), np.int64)
    out = np.empty((6, 4), np.float32)
    assert lib.dhr_score_rows(ix._h, C.byref(qb), 0, rows.ctypes.data, out.ctypes.data, _lib.MEM_HOST, None) < 0
    assert lib.dhr_score_rows(ix._h, C.byref(qb), 4, None, out.ctypes.data, _lib.MEM_HOST, None) < 0
    assert lib.dhr_score_rows(ix._h, C.byref(qb), 4, rows.ctypes.data, None, _lib.MEM_HOST, None) < 0
    assert lib.dhr_score_rows(ix._h, C.byref(qb), 4, rows.ctypes.data, out.ctypes.data, 9, None) < 0           # an unknown memory kind is not "device"
    assert lib.dhr_search_rerank(ix._h, C.byref(qb), C.byref(qb), 100, 50, hs.ctypes.data, hr.ctypes.data, 9, None) < 0
    arr = (C.c_void_p * 1)(ix._h)
    assert lib.dhr_search_sharded_local(arr, 1, C.byref(qb), 50, hs.ctypes.data, hr.ctypes.data, 9, None) < 0
    assert lib.dhr_search_sharded_local(arr, 0, C.byref(qb), 50, hs.ctypes.data, hr.ctypes.data, _lib.MEM_HOST, None) < 0
    cb = np.zeros((4, 16, 2), np.float32); codes = np.zeros((10, 4), np.uint8)
    hp = C.c_void_p()
    assert lib.dhr_pq_create(0, 9, 10, 8, 4, 4, cb.ctypes.data, codes.ctypes.data, 0, C.byref(hp)) < 0 and not hp.value
    assert lib.dhr_pq_create(0, _lib.MEM_HOST, 10, 8, 3, 4, cb.ctypes.data, codes.ctypes.data, 0, C.byref(hp)) < 0 and not hp.value      # d no multiple of M
    assert lib.dhr_pq_decode_nbits(0, 9, codes.ctypes.data, 10, 8, 4, 4, cb.ctypes.data, out.ctypes.data, 8, None) < 0
    lex = np.zeros((2, 16), np.float32); dv = np.zeros((2, 8), np.float32); di = np.zeros((2, 8), np.uint8)
    assert lib.dhr_densify(0, 9, lex.ctypes.data, _lib.VAL_F32, 16, 2, 16, 0, 8, dv.ctypes.data, _lib.VAL_F32, 8, di.ctypes.data, _lib.idx_code(di.dtype), 8, None) < 0
    assert lib.dhr_densify(0, _lib.MEM_HOST, lex.ctypes.data, _lib.VAL_F32, 16, 2, 16, 0, 5, dv.ctypes.data, _lib.VAL_F32, 8, di.ctypes.data, _lib.idx_code(di.dtype), 8, None) < 0
    assert lib.dhr_index_set_param(ix._h, 999, 1) < 0 and lib.dhr_index_set_param(None, _lib.PARAM_CAND_CAP, 1024) < 0
    for prm, val in ((_lib.PARAM_LIST_STRIDE, 256), (_lib.PARAM_LIST_STRIDE, 1025), (_lib.PARAM_CAND_CAP, 1023), (_lib.PARAM_SAMPLE_PERIOD, 257), (_lib.PARAM_MAIN_CHUNKS, 0),
                     (_lib.PARAM_AUX_CUS, 12), (_lib.PARAM_SAMPLE_SHARE, 0), (_lib.PARAM_MAX_GROWTH, 0), (_lib.PARAM_FIRST_ROWS, -1), (_lib.PARAM_GEMM_VARIANT, 3)):
        assert lib.dhr_index_set_param(ix._h, prm, val) < 0, (prm, val)
    assert lib.dhr_index_save(ix._h, b"/nonexistent_dir/x.dhr", None, 0) < 0
    h = C.c_void_p()
    assert lib.dhr_index_load(b"/nonexistent_dir/x.dhr", 0, -1, C.byref(h)) < 0 and not h.value
    # ... and the handle is as good as before
    s1, r1 = ix.search(q32, qi, 50)
    ix.close()
    np.testing.assert_array_equal(r1, r0)
    np.testing.assert_array_equal(s1, s0)


def test_host_corpus_beyond_2_32_elements(G):
    """The reference hands over HOST arrays (the unpickled index): 2.9 M rows x (768 + 768) fp16 = 4.45e9 elements (8.9 GB; 2.2e9 index bytes) cross
    every 32-bit offset of the host ingest (staged blocks, the 2-D copy of the index array).  The index built from the host arrays answers bit for bit
    like the one built from the same data on the device, the last rows of the corpus are where the best scores are, and the returned scores are the float64
    scores of their rows recomputed here."""
    import torch
    n, d, q, k = 2_900_000, 768, 8, 100
    rng = np.random.default_rng(5)
    blk = 100_000
    base_v = (np.abs(rng.standard_normal((blk, 2 * d), dtype=np.float32)) * 0.2).astype(np.float16)
    base_v[:, d:] = (rng.standard_normal((blk, d), dtype=np.float32) * 0.1).astype(np.float16)
    base_i = rng.integers(0, 6, (blk, d)).astype(np.uint8)
    cv = np.empty((n, 2 * d), np.float16)
    ci = np.empty((n, d), np.uint8)
    for lo in range(0, n, blk):
        cv[lo:lo + blk] = base_v
        ci[lo:lo + blk] = base_i
    # every row its own: a ramp in one ungated column that the queries weigh positively -- the LAST rows (beyond 2^32 elements) score highest
    ramp = (np.arange(n, dtype=np.float32) / n * 60.0).astype(np.float16)
    cv[:, d] = ramp
    qv = (np.abs(rng.standard_normal((q, 2 * d), dtype=np.float32)) * 0.2).astype(np.float32)
    qv[:, d:] = rng.standard_normal((q, d), dtype=np.float32) * 0.1
    qv[:, d] = 3.0
    qi = rng.integers(0, 6, (q, d)).astype(np.uint8)
    ix_h = G.GipIndex(cv, ci)
    try:
        s_h, r_h = ix_h.search(qv, qi, k)
    finally:
        ix_h.close()
    dv, di = torch.empty((n, 2 * d), dtype=torch.float16, device="cuda"), torch.empty((n, d), dtype=torch.uint8, device="cuda")
    for lo in range(0, n, 500_000):
        dv[lo:lo + 500_000] = torch.from_numpy(cv[lo:lo + 500_000]).cuda()
        di[lo:lo + 500_000] = torch.from_numpy(ci[lo:lo + 500_000]).cuda()
    ix_d = G.GipIndex(dv, di)
    try:
        s_d, r_d = ix_d.search(qv, qi, k)
    finally:
        ix_d.close()
    np.testing.assert_array_equal(r_h, r_d)
    np.testing.assert_array_equal(s_h, s_d)
    assert (r_h >= (1 << 32) // (2 * d)).all(), "the best rows are the last ones"
    for i in range(q):
        rows = r_h[i]
        ex = O.gip_scores_f64(qv[i], qi[i], cv[rows].astype(np.float32), ci[rows])
        np.testing.assert_allclose(s_h[i], ex.astype(np.float32), rtol=0, atol=1e-6 * float(np.abs(ex).max()))
        # ... and no row of the last 300 000 outside the list beats its k-th score
        tail = slice(n - 300_000, n)
        ext = O.gip_scores_f64(qv[i], qi[i], cv[tail].astype(np.float32), ci[tail])
        O.check_topk(rows - (n - 300_000), s_h[i], ext, k)


def test_integration_md_stub_runs_as_printed(G):
    """The ctypes stub INTEGRATION.md section 2 shows a dhr maintainer is executed AS PRINTED (the first ```python block of the file, the library path
    aside) against the oracle: a stub that cannot run is worse than none (round 6: it passed 64-bit addresses without argtypes)."""
    import re
    from types import SimpleNamespace
    from dhr_amd import _lib, synth
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    code = re.search(r"```python\n(.*?)```", text, re.S).group(1)
    _lib.load()
    code = code.replace('C.CDLL("libdhr_hip.so")', 'C.CDLL(%r)' % os.environ.get("DHR_HIP_LIB", os.path.join(root, "dhr_amd", "csrc", "libdhr_hip.so")))
    ns = {}
    exec(compile(code, "INTEGRATION.md", "exec"), ns)
    cv, ci, qv, qi = synth.make_pair(61, 5000, 7, 64, 32)
    q32 = qv.astype(np.float32)
    qids = ["q%d" % i for i in range(7)]
    res, sc = ns["GIP_retrieval"](qids, q32, qi, cv, ci, SimpleNamespace(emb_dim=64, topk=30))
    c32 = cv.astype(np.float32)
    for i, qid in enumerate(qids):
        O.check_topk(np.array(res[qid]), np.array(sc[qid], np.float32), O.gip_scores_f64(q32[i], qi[i], c32, ci), 30)


def test_corrupted_index_files_are_statuses(G, monkeypatch):
    """A slice of tools/fuzz_index_file.py: byte flips / extreme values in the header region, truncations, garbage behind a valid magic -- dhr_index_file_info
    and dhr_index_load answer with a status, a file whose damage the header cannot see loads and searches without a crash."""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    import fuzz_index_file
    monkeypatch.setattr(sys, "argv", ["fuzz_index_file.py", "400", "5"])
    fuzz_index_file.main()


def test_degenerate_inputs(G, monkeypatch):
    """tools/degenerate.py: all-zero corpus / queries, identical rows (all ties -> row ascending), k == n, one row, fp16 maxima and subnormals,
    all-negative values, one non-zero column -- both images of the gated half, against the oracle."""
    import os, sys
    monkeypatch.setenv("DHR_GATED_I8", "0")      # (the tool sets the variable per case: restored when the test ends)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    import degenerate
    degenerate.main()


def test_staged_search_call_sequences(G, monkeypatch):
    """A slice of tools/fuzz_staged.py: the staged search calls (pre / begin / begin_rest / mid / finish) in ANY order, mixed with the calls that share
    the handle's workspace, with plausible and implausible thresholds -- statuses, never a crash; a protocol-conforming staged search returns the exact
    top-k, a plain search afterwards equals the reference."""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    import fuzz_staged
    monkeypatch.setattr(sys, "argv", ["fuzz_staged.py", "150", "9"])
    fuzz_staged.main()


def test_staged_call_that_fails_closes_the_staged_search(G):
    """A staged entry point that returns an error leaves NO staged search open on the handle: dhr_search_finish fails half-way (the host
    allocation hook of test_allocation_failures_with_a_device: DHR_ERR_NOMEM, nothing on the device fails), so its workspace is half-consumed
    and a second dhr_search_finish must be refused like one without a begin; a fresh begin -> finish on the same handle gives the oracle's result."""
    import torch
    from dhr_amd import synth, _lib
    from dhr_amd import dist as D
    lib = _lib.load()
    cv, ci, qv, qi = synth.make_pair(57, 40_000, 8, 64, 8)
    q, k = qv.astype(np.float32), 100
    ix = G.GipIndex(cv, ci)
    try:
        ix.set_param(_lib.PARAM_SAMPLE_PERIOD, 4)
        r = ix.union_rank(k)
        assert r > 0 and ix.sample_rank(k) == r           # sampled: dhr_search_finish has the main pass to run

        def begin():
            return D.common_threshold(torch.stack([ix.search_begin(q, qi, k)]), r)
        tau = begin()
        lib.dhr_debug_fail_alloc(1)
        try:
            with pytest.raises(_lib.DhrError) as e:
                ix.search_finish(tau)
        finally:
            lib.dhr_debug_fail_alloc(0)
        assert e.value.status == _lib.ERR_NOMEM and "memory" in str(e.value), e.value
        with pytest.raises(_lib.DhrError, match="dhr_search_finish without a matching dhr_search_begin") as e:
            ix.search_finish(tau)
        assert e.value.status == _lib.ERR_INVALID
        scores, rows, count = ix.search_finish(begin())
        scores, rows, count = scores.cpu().numpy(), rows.cpu().numpy(), count.cpu().numpy()
        assert (count >= k).all(), count
        c32 = cv.astype(np.float32)
        for i in range(len(q)):
            O.check_topk(rows[i], scores[i], O.gip_scores_f64(q[i], qi[i], c32, ci), k)
    finally:
        ix.close()


def test_random_mode_configurations(G, monkeypatch):
    """A slice of tools/stress_modes.py: the entry points beside the plain search (two-stage modes on the device, dhr_score_rows, the
    index file round trip, the one-process sharded search over ragged shards, the shard reduces on the device and on the host) on
    random shapes / dtypes / signs / bucket counts / k1 / k, each against the oracle's float64 scores and parity rules."""
    import os, sys
    monkeypatch.setenv("DHR_GATED_I8", "0")      # (the tool sets the variable per case: restored when the test ends)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    import stress_modes
    monkeypatch.setattr(sys, "argv", ["stress_modes.py", "60", "3"])
    stress_modes.main()


def test_bench_two_ranks_share_one_gpu():
    """bench.py's N>1 path end to end (torch.distributed.run, staged sharded search, collectives, JSON line) with two
    ranks on ONE GPU over gloo (DHR_BENCH_SINGLE_DEVICE=1, testing mode); the line must carry the contract's fields
    and bench.py's own property check of the sharded result (--full) must have passed (it raises otherwise)."""
    import json, os, subprocess, sys
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    env = dict(os.environ, DHR_BENCH_SINGLE_DEVICE="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29533", "bench.py", "--gpus", "2", "--steps", "1", "--warmup", "1", "--full", "--dist-backend", "gloo",
           "--n-docs", "700000", "--n-queries", "512"]
    out = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    j = json.loads(line)
    assert j["n_gpus"] == 2 and j["scaling"] == "strong" and j["value"] > 0 and j["unit"] == "queries/s"
    assert j["config"]["parallelism"] == "rowshard2+allgather"
    pc = j["parity_check"]                               # the sharded result's property check ran on both ranks
    assert pc["sorted"] and pc["distinct_rows"] and pc["scores_equal_exact_rescoring"] and pc["rows_beating_kth_outside_list"] == 0


def test_bench_plain_run_dumps_outputs(tmp_path):
    """A plain bench run (no --full) times its steps and does nothing the headline figure does not need; --dump-outputs writes the host
    result lists of the last timed step.  The lists are the exact top-k of bench.py's own seeded inputs (regenerated here with
    bench.gen_rows, checked against the float64 oracle), and a second run with another --steps writes the same arrays."""
    import json, os, subprocess, sys
    import torch
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    n, nq, k = 60_000, 48, 100
    dumps = []
    for steps in (2, 3):
        d = tmp_path / ("out%d" % steps)
        cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--n-docs", str(n), "--n-queries", str(nq),
               "--topk", str(k), "--dump-outputs", str(d)]
        out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        assert j["steps"] == steps and j["ms_per_step"] > 0 and j["value"] > 0 and j["unit"] == "queries/s" and j["higher_is_better"] is True
        assert j["metric"].startswith("queries/sec") and j["dtype"]
        for key in ("cpu_baseline", "parity_check", "two_stage", "other_configs", "device_resident"):
            assert key not in j, key
        assert j["roofline"]["achieved_kernel_alone"] is None and j["roofline"]["achieved"] > 0
        assert sorted(os.listdir(d)) == ["rows.npy", "scores.npy"] and j["outputs"]["queries"] == nq
        dumps.append({name: np.load(d / (name + ".npy")) for name in ("scores", "rows")})
    for name in ("scores", "rows"):
        assert dumps[0][name].dtype == np.float32 and dumps[0][name].shape == (nq, k)
        assert np.array_equal(dumps[0][name], dumps[1][name]), name
    if root not in sys.path:
        sys.path.insert(0, root)
    import bench
    from dhr_amd import synth
    dev = torch.device("cuda", 0)
    cv, ci = bench.gen_rows(torch, synth, dev, 1237, 0, n, 768, 768, 30, 90, False, dup=True)
    qv, qi = bench.gen_rows(torch, synth, dev, 1237 + 999_983, 0, nq, 768, 768, 4, 12, False)
    c32, ci, q32, qi = cv.float().cpu().numpy(), ci.cpu().numpy(), qv.float().cpu().numpy(), qi.cpu().numpy()
    del cv, qv
    for i in range(0, nq, 6):
        O.check_topk(dumps[0]["rows"][i], dumps[0]["scores"][i], O.gip_scores_f64(q32[i], qi[i], c32, ci), k)


def test_bench_real_data_leg(tmp_path):
    """bench.py --index-path / --query-path / --qrels: the timed search on an index + query set in the reference's own record layout, and the
    second half of BASELINE.json's metric (nDCG@10; MRR@10, R@1000) computed from the timed search's lists.  The qrels are built from the
    float64 oracle (the true best row of a query has rel 2, the next two rel 1), so the expected values are known: an exact search must
    score nDCG@10 = MRR@10 = R@1000 = 1."""
    import json, os, subprocess, sys
    from dhr_amd import synth
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    cv, ci, qv, qi = synth.make_pair(77, 40_000, 12, 768, 64)
    docids = ["D%d" % (3 * i + 1) for i in range(cv.shape[0])]
    qids = ["Q%d" % i for i in range(qv.shape[0])]
    dump_pickle(str(tmp_path / "corpus.index.pt"), cv, ci, docids)
    dump_pickle(str(tmp_path / "queries.pt"), qv, qi, qids)
    c32 = cv.astype(np.float32)
    with open(tmp_path / "qrels.tsv", "w") as f:
        for i, qid in enumerate(qids):
            ex = O.gip_scores_f64(qv[i].astype(np.float32), qi[i], c32, ci)
            top = O.topk_desc(ex, 3)
            for j, r in enumerate(top):
                f.write("%s\t0\t%s\t%d\n" % (qid, docids[int(r)], 2 if j == 0 else 1))
            f.write("%s\t0\t%s\t0\n" % (qid, docids[int(np.argmin(ex))]))
    cmd = [sys.executable, "bench.py", "--steps", "2", "--warmup", "1", "--full", "--quick", "--cpu-rows", "20000", "--topk", "100", "--index-path", str(tmp_path / "corpus.index.pt"),
           "--query-path", str(tmp_path / "queries.pt"), "--qrels", str(tmp_path / "qrels.tsv"), "--emb-dim", "768"]
    out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert j["data"].startswith("real") and j["value"] > 0 and "other_configs" not in j
    e = j["effectiveness"]
    assert e["queries_evaluated"] == 12 and e["nDCG@10"] == 1.0 and e["MRR@10"] == 1.0 and e["R@1000"] == 1.0, e
    assert j["parity_check"]["failed"] == 0 and "gemm_filter" in j["roofline"]["kernel"]


def test_bench_rccl_bring_up_hangs_on_one_rank():
    """The N > 1 bench when the bring-up of the library's RCCL communicator goes wrong on ONE rank: two ranks on one GPU, the RCCL trial
    forced (DHR_BENCH_FORCE_RCCL_TRIAL), rank 1 never reaches dhr_comm_create (DHR_TEST_COMM_HANG_RANK) while rank 0 really sits in
    ncclCommInitRank waiting for it.  The watchdog must fire, both ranks must degrade to the host transport, and the run must finish
    with a verified result -- not hang (round-4 review: bench.py's trial / fallback had a deadlock shape)."""
    import json, os, subprocess, sys
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    env = dict(os.environ, DHR_BENCH_SINGLE_DEVICE="1", DHR_BENCH_FORCE_RCCL_TRIAL="1", DHR_TEST_COMM_HANG_RANK="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29537", "bench.py", "--gpus", "2", "--steps", "1", "--warmup", "1", "--full", "--dist-backend", "gloo",
           "--n-docs", "300000", "--n-queries", "256", "--rccl-timeout", "20"]
    out = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert j["sharded_transport"] == "host" and j["n_ranks_seen_by_rccl"] == 0
    assert "dropped on every rank" in j["config"]["collectives"]
    pc = j["parity_check"]
    assert pc["sorted"] and pc["distinct_rows"] and pc["scores_equal_exact_rescoring"] and pc["rows_beating_kth_outside_list"] == 0


def test_score_rows_after_a_smaller_batch(G):
    """A batch that re-uses a larger batch's workspace sets the ACTIVE query count; dhr_score_rows took an early return that did not
    (round-4 advisor): search(large) -> search(small) -> score_rows(medium) prepared only the small batch's rows and scored the other
    queries against stale operand rows."""
    from dhr_amd import synth
    cv, ci, qv, qi = synth.make_pair(77, 6000, 700, 768, 64)
    q32 = qv.astype(np.float32)
    ix = G.GipIndex(cv, ci)
    ix.search(q32, qi, 10)                        # 700 queries -> workspace of 768 rows
    ix.search(q32[:3], qi[:3], 10)                # 3 queries  -> active count 256
    rng = np.random.default_rng(5)
    rows = rng.integers(0, 6000, (600, 7)).astype(np.int64)
    perm = rng.permutation(700)[:600]             # different queries in rows 0..599 than the first search left there
    got = ix.score_rows(q32[perm], qi[perm], rows)
    ix.close()
    c32 = cv.astype(np.float32)
    for i in (0, 1, 255, 256, 300, 511, 512, 599):
        ex = O.gip_scores_f64(q32[perm[i]], qi[perm[i]], c32, ci)[rows[i]]
        np.testing.assert_allclose(got[i], ex.astype(np.float32), rtol=1e-6, atol=1e-6)


def test_config1_bm25_full_query_set(G):
    """BASELINE config 1 at its full query count: 100 k DLR-only BM25-like passages (int16 whole-word slice index), Q = 6 980,
    top-1000; the whole batch is searched, a spread sample of the queries is checked against the oracle's float64 scores."""
    from dhr_amd import synth
    cv, ci, qv, qi = synth.make_pair(1234 + 1, 100_000, 6980, 768, 0, kind="bm25")
    q32 = qv.astype(np.float32)
    ix = G.GipIndex(cv, ci)
    scores, rows = ix.search(q32, qi, 1000)
    st = ix.stats()
    ix.close()
    assert scores.shape == (6980, 1000) and np.all(rows >= 0)
    assert np.all(np.diff(scores, axis=1) <= 0)
    c32 = cv.astype(np.float32)
    for i in range(0, 6980, 349):                      # 20 queries over the whole batch
        ex = O.gip_scores_f64(q32[i], qi[i], c32, ci)
        O.check_topk(rows[i], scores[i], ex, 1000)
    print({k: st[k] for k in ("phases", "candidates_bound", "candidates_exact", "total_ms")})


def _fake_world_search_any(G, shards, q, qi, k):
    """dhr_amd.dist.sharded_search with the collectives replaced by in-process tensor ops (one GPU, S shards), INCLUDING its
    fallback for shards that cannot be sampled uniformly (tiny or unequal shards: local thresholds, k > rows of a shard)."""
    import torch
    from dhr_amd import dist as D
    rs = [s.sample_rank(k) for s in shards]
    if rs[0] == 0 or any(r != rs[0] for r in rs):
        outs = [s.search(q, qi, k, out_device=True) for s in shards]
        ms, mr = D.merge_topk(torch.cat([o[0] for o in outs], 1), torch.cat([o[1] for o in outs], 1), k)
        return ms.cpu().numpy(), mr.cpu().numpy(), "local"
    ms, mr, n_failed, _ = _fake_world_search(G, shards, q, qi, k)
    return ms, mr, "common-threshold (%d failed)" % n_failed


def test_config5_beir_sizes_sharded_8(G):
    """BASELINE config 5's corpus sizes (the 13 public BEIR corpora, 3.6 k ... 5.4 M documents; hybrid 768 + 128) through the
    8-shard path on one GPU: the merged result must be bit-identical to the unsharded search of the same corpus, for every
    size -- including the corpora where a shard holds fewer rows than k (nfcorpus: 454 rows per shard, k = 1000; the reference's
    torch.topk raises there, gip_retrieval.py:123, the build pads).  The small corpora are also checked against the oracle, the
    large ones through size-independent properties (exact rescoring of every returned row, no sampled outsider beats the k-th)."""
    import torch
    import bench
    from dhr_amd import synth
    dev = torch.device("cuda", 0)
    k, nq, ns = 1000, 16, 8
    for name, n, _ in bench.BEIR:
        cv, ci = bench.gen_rows(torch, synth, dev, 4300 + (n % 97), 0, n, 768, 128, 30, 90, False)
        qv, qi = bench.gen_rows(torch, synth, dev, 99, 0, nq, 768, 128, 4, 12, False)
        full = G.GipIndex(cv, ci)
        kk = min(k, n)
        fs, fr = full.search(qv, qi, kk, out_device=True)
        shards = []
        for sh in range(ns):
            lo, hi = G.shard_bounds(n, ns, sh)
            shards.append(G.GipIndex(cv[lo:hi], ci[lo:hi], row_offset=lo))
        ms, mr, how = _fake_world_search_any(G, shards, qv, qi, kk)
        from dhr_amd import dist as D
        cs, cr = D.search_sharded_local(shards, qv, qi, kk)            # the product path: dhr_search_sharded_local (C ABI)
        np.testing.assert_array_equal(cr.cpu().numpy(), mr, err_msg=name)
        np.testing.assert_array_equal(cs.cpu().numpy(), ms, err_msg=name)
        for s in shards:
            s.close()
        fs_h, fr_h = fs.cpu().numpy(), fr.cpu().numpy()
        np.testing.assert_array_equal(mr, fr_h, err_msg=name)
        np.testing.assert_array_equal(ms, fs_h, err_msg=name)
        q32 = qv.cpu().numpy().astype(np.float32)
        qih = qi.cpu().numpy()
        if n <= 60_000:
            c32, cih = cv.cpu().numpy().astype(np.float32), ci.cpu().numpy()
            for i in range(nq):
                O.check_topk(fr_h[i], fs_h[i], O.gip_scores_f64(q32[i], qih[i], c32, cih), kk)
        else:
            assert np.all(np.diff(fs_h, axis=1) <= 0) and all(len(set(r.tolist())) == kk for r in fr_h)
            np.testing.assert_array_equal(full.score_rows(q32, qih, fr_h), fs_h)         # an independent code path (dhr_score_rows)
            rnd = np.random.default_rng(n).integers(0, n, (nq, 20_000)).astype(np.int64)
            outsider = full.score_rows(q32, qih, rnd)
            for i in range(nq):
                assert not np.any((outsider[i] > fs_h[i, -1]) & ~np.isin(rnd[i], fr_h[i])), name
        full.close()
        del cv, ci
        torch.cuda.empty_cache()
        print(name, n, how)


def test_query_chunking_same_result(G, golden, monkeypatch):
    """The host mirror hands the library the query set in slices (QUERY_CHUNK; the reference loops per query and takes any number):
    results must not depend on the slice size, in the brute-force, two-stage and dense-only entry points."""
    info, _, _ = golden.case("F3_hyb_brute_k100")
    d = golden.inputs("hyb")
    q, qi = O.prepare_queries(d["qv"], d["qi"], 768, 1.0)
    qids = list(d["qids"])
    args2 = case_args(dict(topk=50, theta=0.3, rerank=True, agip_topk=300))
    ref = (G.GIP_retrieval(qids, q, qi, d["cv"], d["ci"], case_args(info)), G.GIP_retrieval(qids, q, qi, d["cv"], d["ci"], args2),
           G.IP_retrieval(qids, q, d["cv"], case_args(dict(topk=20))))
    monkeypatch.setattr(G, "QUERY_CHUNK", 5)
    got = (G.GIP_retrieval(qids, q, qi, d["cv"], d["ci"], case_args(info)), G.GIP_retrieval(qids, q, qi, d["cv"], d["ci"], args2),
           G.IP_retrieval(qids, q, d["cv"], case_args(dict(topk=20))))
    assert ref == got


@pytest.mark.parametrize("kind", ["hybrid", "dense", "structured", "tiny"])
def test_search_sharded_local_c_abi(G, kind, gated_image):
    """dhr_search_sharded_local (one process, S shard handles; the same sharded_core as the RCCL entry point, gathers by device
    copies) == the unsharded search, bit for bit: common-threshold path (hybrid, dense), its failure repair (structured: every
    high-scoring row sits in sample tiles of shard 0), and the local-threshold path (tiny shards, k > rows of a shard)."""
    from dhr_amd import synth, _lib, dist as D
    k = 1000
    period = 4
    if kind == "hybrid":
        n, ns = 400_000, 4
        cv, ci, qv, qi = synth.make_pair(22, n, 12, 768, 64)
    elif kind == "dense":
        n, ns = 400_000, 4
        cv, ci, qv, qi = synth.make_pair(23, n, 12, 0, 256, kind="dense")
    elif kind == "structured":
        n, ns, period = 401_408, 2, 16          # both shards start on a multiple of 16 tiles (see test_staged_sharded_search_failure_path)
        cv, qv = _structured_corpus(n, 0)
        ci = qi = None
    else:
        n, ns, k = 3_000, 8, 500
        cv, ci, qv, qi = synth.make_pair(24, n, 9, 768, 128)
    q32 = qv.astype(np.float32)
    full = G.GipIndex(cv, ci)
    fs, fr = full.search(q32, qi, k)
    full.close()
    shards = []
    for sh in range(ns):
        lo, hi = G.shard_bounds(n, ns, sh)
        shards.append(G.GipIndex(cv[lo:hi], None if ci is None else ci[lo:hi], row_offset=lo))
        shards[-1].set_param(_lib.PARAM_SAMPLE_PERIOD, period)
    try:
        for q_in, qi_in in ((q32, qi), (qv, qi)):                      # fp32 host batch, fp16 host batch
            ss, sr = D.search_sharded_local(shards, q_in, qi_in, k)
            np.testing.assert_array_equal(sr.cpu().numpy(), fr)
            np.testing.assert_array_equal(ss.cpu().numpy(), fs)
        import torch
        qd = torch.from_numpy(q32).cuda()
        qid = None if qi is None else torch.from_numpy(qi).cuda()
        ss, sr = D.search_sharded_local(shards, qd, qid, k)             # device-resident batch (the failure repair gathers on the device)
        np.testing.assert_array_equal(sr.cpu().numpy(), fr)
        np.testing.assert_array_equal(ss.cpu().numpy(), fs)
    finally:
        for s in shards:
            s.close()


def test_search_sharded_local_prefix_and_repair(G):
    """Five shards and k = 300: the lists of the last all-gather travel as PREFIXES (prefix_len: kk = 256 < k, the device prefix kernel), and on
    the structured corpus -- every high-scoring row sits in a sample tile of its shard -- the common threshold comes out too high, the count
    check fails every query and the device repair path redoes them; the result equals the unsharded search bit for bit.  528 tiles per shard:
    the fewest that keep a shard sampleable at period 16 (>= 32 * 16 tiles behind the head) with every shard starting on a multiple of 16 tiles."""
    import torch
    from dhr_amd import _lib, dist as D
    ns, k, period = 5, 300, 16
    n = ns * 528 * 256
    cv, qv = _structured_corpus(n, 0, period)
    q32 = qv.astype(np.float32)
    full = G.GipIndex(cv, None)
    fs, fr = full.search(q32, None, k)
    full.close()
    shards = []
    for sh in range(ns):
        lo, hi = G.shard_bounds(n, ns, sh)
        assert lo % (period * 256) == 0
        shards.append(G.GipIndex(cv[lo:hi], None, row_offset=lo))
        shards[-1].set_param(_lib.PARAM_SAMPLE_PERIOD, period)
    try:
        ss, sr = D.search_sharded_local(shards, torch.from_numpy(q32).cuda(), None, k)      # device-resident batch: the repair gathers on the device
        repairs = _lib.load().dhr_debug_sharded_repairs()
        np.testing.assert_array_equal(sr.cpu().numpy(), fr)
        np.testing.assert_array_equal(ss.cpu().numpy(), fs)
        assert repairs > 0
    finally:
        for s in shards:
            s.close()


def test_search_sharded_rccl_single_rank(G):
    """dhr_comm_* + dhr_search_sharded through a real RCCL communicator of world size 1 (all this one-GPU box can hold): the
    collective entry point, its scratch arena and the result delivery; equals dhr_search."""
    from dhr_amd import synth, dist as D
    cv, ci, qv, qi = synth.make_pair(25, 120_000, 10, 768, 64)
    q32 = qv.astype(np.float32)
    ix = G.GipIndex(cv, ci)
    try:
        fs, fr = ix.search(q32, qi, 1000)
        comm = D.ShardComm(0)
        assert comm.world == 1 and comm.rank == 0
        comm.close()
        for _ in range(2):                                             # second call reuses the grown arena
            ss, sr = D.sharded_search(ix, q32, qi, 1000)
            np.testing.assert_array_equal(sr.cpu().numpy(), fr)
            np.testing.assert_array_equal(ss.cpu().numpy(), fs)
    finally:
        ix.close()


def test_two_stage_agip_topk_beyond_16384(G):
    """--theta 0.3 --rerank --agip_topk 20000 (stage-1 list beyond the LDS merge) against the oracle, two-stage tie-band rule."""
    from dhr_amd import synth
    cv, ci, qv, qi = synth.make_pair(61, 30_000, 3, 768, 128)
    q32 = qv.astype(np.float32)
    info = dict(topk=200, theta=0.3, rerank=True, agip_topk=20000)
    qids = ["a", "b", "c"]
    res, sc = G.GIP_retrieval(qids, q32, qi, cv, ci, case_args(info))
    c32 = cv.astype(np.float32)
    for i, qid in enumerate(qids):
        _check_theta_mode(info, q32[i], qi[i], c32, ci, res[qid], sc[qid])


def _i8_pair(G, cv, ci, qv32, qi, k, *, dense_only_opt=False, ungated=False):
    """The same search with fp16 and with int8 ungated stages: identical rows, scores and both exact."""
    from dhr_amd import _lib
    lib = _lib.load()
    out = []
    try:
        for opt in (0, 1):
            _lib.check(lib.dhr_set_option(_lib.OPT_DENSE_I8, opt), "set_option")
            ix = G.GipIndex(cv, ci)
            assert int(ix.info(_lib.INFO_DENSE_I8)) == opt
            ix.set_param(_lib.PARAM_PROFILE, 1)
            s, r = ix.search(qv32, None if ungated else qi, k)
            out.append((s, r, ix.stats(), ix.info(_lib.INFO_TILE_BYTES)))
            ix.close()
    finally:
        _lib.check(lib.dhr_set_option(_lib.OPT_DENSE_I8, -1), "set_option")
    (s0, r0, st0, b0), (s1, r1, st1, b1) = out
    np.testing.assert_array_equal(r0, r1)
    np.testing.assert_array_equal(s0, s1)
    c32 = cv.astype(np.float32)
    for i in range(min(4, qv32.shape[0])):
        ex = O.gip_scores_f64(qv32[i], None if (ungated or qi is None) else qi[i], c32, None if ungated else ci)
        O.check_topk(r1[i, :min(k, len(ex))], s1[i, :min(k, len(ex))], ex, k, atol=max(1e-3, 1e-6 * float(np.abs(ex).max())))
    return st0, st1, b0, b1


def test_dense_i8_equals_fp16_hybrid(G):
    """int8 image of the ungated columns (v_mfma_i32_32x32x32_i8 stages, accumulators started at 2^23 + 2^22): the survivors are a
    superset, the results identical; the operand images shrink by the ungated half."""
    from dhr_amd import synth
    cv, ci, qv, qi = synth.make_pair(21, 60_000, 40, 768, 768)
    st0, st1, b0, b1 = _i8_pair(G, cv, ci, qv.astype(np.float32), qi, 1000)
    assert b1 < b0 and st1["candidates_bound"] >= st0["candidates_bound"]
    print("bound candidates fp16 / int8:", st0["candidates_bound"], st1["candidates_bound"], "exact:", st0["candidates_exact"], st1["candidates_exact"])
    # ungated batch (--IP stage 1) over the gated int8 index, and a width that needs zero padding of the int8 stages
    _i8_pair(G, cv[:20_000], ci[:20_000], qv[:9].astype(np.float32), qi[:9], 300, ungated=True)
    cv2 = np.ascontiguousarray(np.concatenate([cv[:9000, :768], cv[:9000, 768:768 + 200]], axis=1))
    qv2 = np.ascontiguousarray(np.concatenate([qv[:7, :768], qv[:7, 768:768 + 200]], axis=1))
    _i8_pair(G, cv2, ci[:9000], qv2.astype(np.float32), qi[:7], 100)


def test_dense_i8_dense_only_index(G):
    from dhr_amd import synth
    cv, _, qv, _ = synth.make_pair(22, 40_000, 30, 0, 768, kind="dense")
    from dhr_amd import _lib
    lib = _lib.load()
    ix = G.GipIndex(cv, None)
    assert int(ix.info(_lib.INFO_DENSE_I8)) == 0            # default: gated indexes only
    ix.close()
    _i8_pair(G, cv, None, qv.astype(np.float32), None, 100)


@pytest.mark.parametrize("kind", ["spiky_rows", "huge_gated", "zero_dense", "tiny_dense", "one_hot_queries", "fp32_queries", "negative_gated"])
def test_dense_i8_adversarial(G, kind):
    """Inputs that stress the int8 image: rows / queries whose ungated part is one large entry (the query scale is coarsened until
    the integer sums fit the accumulator offset), gated values near the fp16 limit (the scale is raised until they fit in scaled
    units), an all-zero or tiny ungated part, queries that are not fp16-representable, negative gated values (abs mode)."""
    rng = np.random.default_rng(zlib.crc32(kind.encode()) % 1000)
    n, q, d = 6000, 12, 128
    cv = np.abs(rng.standard_normal((n, 2 * d)) * 0.3).astype(np.float16)
    cv[:, d:] = (rng.standard_normal((n, d)) * 0.1).astype(np.float16)
    qv = np.abs(rng.standard_normal((q, 2 * d)) * 0.3).astype(np.float32)
    qv[:, d:] = (rng.standard_normal((q, d)) * 0.1).astype(np.float16)
    ci = rng.integers(0, 6, (n, d)).astype(np.uint8)
    qi = rng.integers(0, 6, (q, d)).astype(np.uint8)
    if kind == "spiky_rows":
        cv[:, d:] = 0
        cv[np.arange(n), d + rng.integers(0, d, n)] = np.float16(40.0)
        cv[::7, d:] = np.float16(40.0)                      # rows with the largest possible int8 norm
        qv[:, d:] = np.float16(3.0)
    elif kind == "huge_gated":
        cv[::5, :d] = np.float16(900.0)
        qv[::2, :d] = 50.0
    elif kind == "zero_dense":
        cv[:, d:] = 0
        qv[3:, d:] = 0
    elif kind == "tiny_dense":
        cv[:, d:] = (rng.standard_normal((n, d)) * 1e-4).astype(np.float16)
        qv[:, d:] = (rng.standard_normal((q, d)) * 1e-4).astype(np.float16)
    elif kind == "one_hot_queries":
        qv[:, d:] = 0
        qv[np.arange(q), d + rng.integers(0, d, q)] = 2.0
    elif kind == "fp32_queries":
        qv = (qv * np.float32(1.0001) + np.float32(1e-5)).astype(np.float32)
    elif kind == "negative_gated":
        cv[::3, :d] *= np.float16(-1)
        qv[::2, :d] *= -1
    _i8_pair(G, cv, ci, qv, qi, 200)


@pytest.mark.parametrize("nbits", [4, 6])
def test_pq_n_bits_below_8(G, tmp_path, monkeypatch, nbits):
    """`--n_bits` < 8 (quantize_index.py:22,29): 2^nbits centroids per sub-quantiser -- training, encoding, decoding and the ADC scan
    against the oracle with the same codebooks; the faiss IndexPQ file carries bit-packed rows; CLI round trip."""
    import pickle
    from dhr_amd import synth
    from dhr_amd.retrieval import quantize_index as QI
    from oracle import pq_oracle as PO
    cv, ci, qv, qi = synth.make_pair(43, 12000, 8, 768, 128)
    q = qv.astype(np.float32)
    ksub = 1 << nbits
    cb, codes, err = QI.train_and_encode(cv, 64, nbits, iters=6)
    assert cb.shape == (64, ksub, 14) and codes.dtype == np.uint8 and int(codes.max()) < ksub
    ecodes = PO.encode(cv[:3000].astype(np.float32), cb)
    assert (ecodes != codes[:3000]).mean() < 2e-3
    ocb = PO.train(cv, 64, iters=6, nbits=nbits)
    assert PO.mse(cv[:4000], cb) <= 1.03 * PO.mse(cv[:4000], ocb)
    np.testing.assert_array_equal(QI.decode(cb, codes), PO.decode(codes, cb).astype(np.float16))
    pix = QI.PqIndex(cb, codes, nbits=nbits)
    try:
        adc = PO.adc_scores(q, codes, cb)
        np.testing.assert_allclose(pix.adc_scores(q).cpu().numpy(), adc, rtol=0, atol=1e-5 * max(1.0, float(np.abs(adc).max())))
        s1, r1 = pix.search(q, 300)
        for i in range(8):
            O.check_topk(r1[i], s1[i], adc[i], 300, atol=1e-4)
    finally:
        pix.close()
    # file: code_size = ceil(64 * nbits / 8) bytes per row, read back identically
    QI.save_pq(str(tmp_path / "pq.idx"), cb, codes, nbits)
    back = QI.load_pq(str(tmp_path / "pq.idx"))
    assert back["nbits"] == nbits and os.path.getsize(tmp_path / "pq.idx") < 12000 * (64 * nbits // 8) + 64 * ksub * 14 * 4 + 256
    np.testing.assert_array_equal(back["codes"], codes)
    np.testing.assert_array_equal(back["codebooks"], cb)
    # CLI with --n_bits
    monkeypatch.chdir(tmp_path)
    with open("q.pt", "wb") as f:
        pickle.dump([qv, qi, ["q%d" % i for i in range(8)]], f, protocol=4)
    with open("c.pt", "wb") as f:
        pickle.dump([cv, ci, ["d%d" % i for i in range(12000)]], f, protocol=4)
    QI.main(["--index_path", "c.pt", "--output_index_path", "pqn_index", "--n_bits", str(nbits)])
    G.main(["--query_emb_path", "q.pt", "--index_path", "c.pt", "--emb_dim", "768", "--PQIP", "--faiss_pq_index_path", "pqn_index",
            "--rerank", "--agip_topk", "400", "--topk", "10", "--output", "pqn.trec"])
    assert len(open("pqn.trec").read().splitlines()) == 80


def test_extrapolated_threshold_failure_is_redone(G, gated_image):
    """DHR_PARAM_PROGRESSIVE_THR = 2: after every main-pass chunk the threshold is raised to the rank extrapolated from the scattered
    fraction of the corpus seen so far.  Adversarial placement: 56 outstanding rows (fewer than k = 64), ALL inside the tiles the
    scattered order visits in the first chunk -- the extrapolation (rank 53 of the seen rows) lands on their score, every later row
    is filtered, fewer than k rows reach the threshold: the verification must fail and the query be redone exactly.  The visiting
    order is restated from search_core.hip (search_core): non-sample position i -> (i * perm_mul) % n_main."""
    import math
    from dhr_amd import _lib
    n, S, k, M = 720_000, 4, 64, 8                      # 2 108 non-sample tiles: the planner allows 8 chunks from 2 048 on
    rng = np.random.default_rng(11)
    cv = (rng.standard_normal((n, 64)) * 0.02).astype(np.float16)
    n_tiles = (n + 255) // 256
    head = 0                                            # no exhaustive head in a sampled search (threshold bootstrap; 1 tile until round 4)
    rest = n_tiles - head
    n_sample = (rest + S - 1) // S
    n_main = rest - n_sample
    perm_mul = int(0.6180339887 * n_main) | 1
    while math.gcd(perm_mul, n_main) != 1:
        perm_mul += 2
    bound1 = min(n_main, -(-int(n_main * 3.0 / 16.0) // 4) * 4)     # chunk 0 of 8: weight 3 of 16, whole tile groups
    first_tiles = []
    for i in range(bound1):
        m = (i * perm_mul) % n_main
        first_tiles.append(head + (m // (S - 1)) * S + m % (S - 1) + 1)
    rows = np.concatenate([np.arange(t * 256, min(n, t * 256 + 256)) for t in first_tiles[:20]])
    boosted = rng.choice(rows, 56, replace=False)
    cv[boosted, 0] = (2.0 + rng.random(56) * 0.1).astype(np.float16)
    qv = np.zeros((3, 64), np.float32)
    qv[:, 0] = 1.0
    qv[:, 1:] = rng.standard_normal((3, 63)).astype(np.float16) * 0.01
    params = [(_lib.PARAM_SAMPLE_PERIOD, S), (_lib.PARAM_MAIN_CHUNKS, M)]
    _, rows2, st2 = _search_check(G, cv, None, qv, None, k, params=params + [(_lib.PARAM_PROGRESSIVE_THR, 2)])
    assert st2["sample_fallback_queries"] >= 3, st2
    assert set(boosted.tolist()) <= set(rows2[0].tolist())
    _, rows1, st1 = _search_check(G, cv, None, qv, None, k, params=params + [(_lib.PARAM_PROGRESSIVE_THR, 1)])
    assert st1["sample_fallback_queries"] == 0
    np.testing.assert_array_equal(rows1, rows2)


def test_dense_i8_outlier_columns(G):
    """A few ungated columns 50x larger than the rest (the outlier dimensions of encoder outputs): the int8 image quantises every column
    in its own units (query-side weights), so the margin -- and with it the number of rescored rows -- stays close to the fp16 image's;
    results identical."""
    from dhr_amd import synth
    cv, ci, qv, qi = synth.make_pair(23, 40_000, 24, 768, 128)
    cv = cv.copy(); qv = qv.copy()
    cv[:, 768 + 5] *= np.float16(50); cv[:, 768 + 77] *= np.float16(30)
    st0, st1, _, _ = _i8_pair(G, cv, ci, qv.astype(np.float32), qi, 200)
    print("exact rescorings fp16 / int8:", st0["candidates_exact"], st1["candidates_exact"])
    assert st1["candidates_exact"] <= 3 * st0["candidates_exact"]


@pytest.mark.parametrize("q,n_in,k", [(5, 16385, 1000), (3, 40000, 5000), (2, 24000, 30000)])
def test_merge_topk_device_beyond_16384_entries(G, q, n_in, k):
    """dhr_merge_topk with more entries per query than one workgroup's LDS holds (e.g. full-k lists of more than 16 shards): two stable
    segmented sorts through global memory; the same (score desc, row asc) order as the host reduce and the oracle, ties, 64-bit rows
    and padding included; k_out > n_in pads."""
    import torch
    from dhr_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(n_in)
    s = np.round(rng.standard_normal((q, n_in)).astype(np.float32), 1) + np.float32(0)        # many exact ties (and no -0.0: the library orders by bit pattern)
    r = (rng.permutation(50_000_000)[: q * n_in].reshape(q, n_in).astype(np.int64) + (1 << 33))     # rows beyond 32 bits
    r[:, -11:] = -1
    s[0, :3] = np.float32("-inf")
    es, er = O.merge_topk([s], [r], k)
    hs, hr = np.empty((q, k), np.float32), np.empty((q, k), np.int64)
    _lib.check(lib.dhr_merge_topk_host(q, n_in, s.ctypes.data, r.ctypes.data, k, hs.ctypes.data, hr.ctypes.data), "host merge")
    np.testing.assert_array_equal(hr, er)
    ds, dr = torch.from_numpy(s).cuda(), torch.from_numpy(r).cuda()
    os_, or_ = torch.empty((q, k), dtype=torch.float32, device="cuda"), torch.empty((q, k), dtype=torch.int64, device="cuda")
    _lib.check(lib.dhr_merge_topk(0, q, n_in, ds.data_ptr(), dr.data_ptr(), k, os_.data_ptr(), or_.data_ptr(), 0), "dev merge")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(or_.cpu().numpy(), er)
    np.testing.assert_array_equal(os_.cpu().numpy(), es)


def test_pq_search_k_beyond_16384(G):
    """IndexPQ.search with k above the LDS select (faiss has no such limit): the global-memory merge, exact top-k of the ADC scores."""
    from dhr_amd import synth
    from dhr_amd.retrieval import quantize_index as QI
    from oracle import pq_oracle as PO
    cv, _, qv, _ = synth.make_pair(47, 60_000, 3, 768, 128)
    q = qv.astype(np.float32)
    cb, codes, _ = QI.train_and_encode(cv, 64, 8, iters=3)
    pix = QI.PqIndex(cb, codes)
    try:
        adc = PO.adc_scores(q, codes, cb)
        for k in (20000, 60000):
            s1, r1 = pix.search(q, k)
            for i in range(3):
                O.check_topk(r1[i], s1[i], adc[i], k, atol=1e-4)
    finally:
        pix.close()


@pytest.mark.parametrize("k", [20000, 10000, 4500])
def test_search_sharded_local_k_beyond_16384(G, k):
    """The sharded search with k above the LDS select / LDS list merge: the shards' lists are reduced by the general device reduce
    (k = 20 000); 4 096 < k <= 16 384: every shard keeps its running list in memory and merges it in place (select_big_kernel)
    under the sampled-rank / agreement protocol of the sharded step."""
    from dhr_amd import synth, _lib, dist as D
    n, ns = 200_000, 4
    cv, ci, qv, qi = synth.make_pair(52, n, 3, 768, 64)
    q32 = qv.astype(np.float32)
    full = G.GipIndex(cv, ci)
    fs, fr = full.search(q32, qi, k)
    full.close()
    shards = []
    for sh in range(ns):
        lo, hi = G.shard_bounds(n, ns, sh)
        shards.append(G.GipIndex(cv[lo:hi], ci[lo:hi], row_offset=lo))
    try:
        ss, sr = D.search_sharded_local(shards, q32, qi, k)
        np.testing.assert_array_equal(sr.cpu().numpy(), fr)
        np.testing.assert_array_equal(ss.cpu().numpy(), fs)
    finally:
        for s in shards:
            s.close()


def test_zero_score_ties_under_sampling(G, gated_image):
    """Queries with fewer than k matching rows: the tail of the list is rows of score 0.0, and the rule (score desc, row asc) puts the
    LOWEST rows there.  The sampled run publishes the r-th best as threshold but must keep the k best rows it saw -- the rows of the
    head and of the sample tiles tie with the final k-th score (a 100 k-row corpus is sampled since the period adapts to the size)."""
    from dhr_amd import synth, _lib
    n, k = 100_000, 1000
    cv, ci, qv, qi = synth.make_pair(77, n, 8, 768, 0, kind="bm25")
    nz = cv > 0
    sl = np.broadcast_to(np.arange(768, dtype=np.int64)[None, :], cv.shape)[nz]
    key = sl * 65536 + (ci.astype(np.int64)[nz] & 0xFFFF)
    uk, cnt = np.unique(key, return_counts=True)
    rare = uk[(cnt >= 3) & (cnt <= 400)]
    rng = np.random.default_rng(5)
    q32 = np.zeros((12, 768), np.float32)
    qidx = np.zeros((12, 768), ci.dtype)
    for i in range(12):
        for kk_ in rng.choice(rare, 2, replace=False):         # two rare words per query: a few hundred matching rows at most
            q32[i, kk_ // 65536] = 1.0 + i
            qidx[i, kk_ // 65536] = kk_ % 65536
    c32 = cv.astype(np.float32)
    ix = G.GipIndex(cv, ci)
    assert ix.sample_rank(k) > 0                                # the search takes the sampled path
    s, r = ix.search(q32, qidx, k)
    st = ix.stats()
    ix.close()
    assert st["sample_fallback_queries"] == 0
    for i in range(12):
        ex = O.gip_scores_f64(q32[i], qidx[i], c32, ci)
        assert (ex > 0).sum() < k
        order = np.lexsort((np.arange(n), -ex))[:k]
        np.testing.assert_array_equal(r[i], order)
        np.testing.assert_array_equal(s[i], ex[order].astype(np.float32))


def test_ungated_batch_deep_candidate_lists(G, force_gated_i8):
    """Plain inner product (--IP stage 1: a batch without an index array) on a GATED index whose rows all score nearly alike, so that
    the filter passes almost every row: one main-pass chunk brings a query far more than 32 768 candidates.  Until round 3 such a
    batch kept the refine-depth bound lists over the shallower key buffer, and a long list overwrote the neighbouring queries' keys
    (found at full size: 62 of 6 980 --IP queries failed their verification per step).  Exact inner products from the oracle."""
    rng = np.random.default_rng(77)
    n, nq, d_dlr, d_cls, k = 150_000, 6, 64, 64, 500
    base = np.abs(rng.normal(0, 1, (1, d_dlr + d_cls))).astype(np.float32)
    cv = (base + rng.normal(0, 2e-3, (n, d_dlr + d_cls)).astype(np.float32))
    cv[:, :d_dlr] = np.abs(cv[:, :d_dlr])
    cv = cv.astype(np.float16)
    ci = rng.integers(0, 39, (n, d_dlr)).astype(np.uint8)
    q = np.abs(rng.normal(0, 1, (nq, d_dlr + d_cls))).astype(np.float16).astype(np.float32)
    ix = G.GipIndex(cv, ci)
    try:
        sc, rows = ix.search(q, None, k)
        st = ix.stats()
        assert st["candidates_bound"] / nq > 40_000, st          # the lists really were deep
        c64 = cv.astype(np.float64)
        for i in range(nq):
            ex = c64 @ q[i].astype(np.float64)
            O.check_topk(rows[i], sc[i], ex, k)
    finally:
        ix.close()


def test_pq_first_stage_beir_size(G):
    """Config 5's quantised-index leg at a BEIR corpus size (quora: 522 931 rows, 768 + 128; parity with faiss UNPINNED): the ADC scan
    over resident codes against the library's own raw ADC scores on the whole corpus (the scan's top-k must be the exact top-k of
    those table sums), a slice of the raw scores against the oracle's table sums, and recall of the reranked result against the
    exact search -- properties that do not depend on the corpus size."""
    import sys
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import bench
    from dhr_amd import synth
    from dhr_amd.retrieval import quantize_index as QI
    from oracle import pq_oracle as PO
    dev = torch.device("cuda", 0)
    n, nq, k1, k = 522_931, 512, 10_000, 100
    cv, ci = bench.gen_rows(torch, synth, dev, 4242, 0, n, 768, 128, 30, 90, False)
    qv, qi = bench.gen_rows(torch, synth, dev, 4242 + 999_983, 0, nq, 768, 128, 4, 12, False)
    cb, codes, err = QI.train_and_encode(cv, 64, 8, iters=4)
    pix = QI.PqIndex(cb, codes)
    ix = G.GipIndex(cv, ci)
    try:
        q = qv.float()
        s1, r1 = pix.search(q, k1, out_device=True)
        assert pix.device_bytes() < n * 64 + 64 * 256 * 14 * 4 + (2 << 30)            # codes + codebooks + the bounded search workspace
        raw = pix.adc_scores(q[:32])                                                    # [32, n] table sums of the library
        top = torch.topk(raw, k1, dim=1)
        for i in range(32):
            got = s1[i].double().cpu().numpy()
            want = top.values[i].double().cpu().numpy()
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-4 * max(1.0, float(np.abs(want).max())))        # same multiset of scores
            kth = float(want[-1])
            inside = raw[i][r1[i]]                                                      # every returned row really has its returned score
            np.testing.assert_allclose(inside.cpu().numpy(), s1[i].cpu().numpy(), rtol=0, atol=1e-4 * max(1.0, abs(kth)))
        # a slice of the raw scores against the oracle's table sums
        sl = slice(100_000, 104_000)
        adc = PO.adc_scores(q[:8].cpu().numpy(), codes[sl].cpu().numpy(), cb.cpu().numpy())
        np.testing.assert_allclose(raw[:8, sl].cpu().numpy(), adc, rtol=0, atol=1e-5 * max(1.0, float(np.abs(adc).max())))
        # --PQIP --rerank: exact GIP on the 10 000 ADC candidates vs the exact search
        se, re_ = ix.search(q, qi, k, out_device=True)
        s2 = ix.score_rows_device(q, qi, r1)
        order = torch.argsort(s2, dim=1, descending=True)[:, :10]
        rr = torch.gather(r1, 1, order)
        rec = np.mean([len(set(rr[i].tolist()) & set(re_[i, :10].tolist())) / 10.0 for i in range(0, nq, 8)])
        assert rec >= 0.9, rec
    finally:
        pix.close(); ix.close()


@pytest.mark.parametrize("name,n,nq", [("fiqa", 57_638, 648), ("quora", 522_931, 512), ("arguana", 8_674, 1_406)])
def test_config5_pq_sharded_8_equals_unsharded(G, name, n, nq):
    """BASELINE config 5 literally -- PQ-quantised index x BEIR corpus sizes x 8 row shards (parity of the PQ stage with faiss UNPINNED):
    the sharded --PQIP --rerank search (dist.pq_sharded_search: per-shard ADC scan, exact global agip_topk cut by bisection on the score
    bits, per-shard exact rerank, all-gather + rank merge of the [Q, k] lists) must return the UNSHARDED search's lists bit for bit --
    one set of codebooks, a shard's codes = its slice of the corpus' codes (gip_retrieval.py:167-231 under the shard arithmetic of
    :292-306; merge.result.py:22-42).  arguana: agip_topk exceeds the rows of every shard AND of the corpus."""
    import sys
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import bench
    from dhr_amd import synth, dist as D
    from dhr_amd.retrieval import quantize_index as QI
    dev = torch.device("cuda", 0)
    k1, k, ns = 10_000, 1000, 8
    seed = 5150 + n % 97
    cv, ci = bench.gen_rows(torch, synth, dev, seed, 0, n, 768, 128, 30, 90, False)
    qv, qi = bench.gen_rows(torch, synth, dev, seed + 999_983, 0, nq, 768, 128, 4, 12, False)
    cb, codes, _ = QI.train_and_encode(cv, 64, 8, iters=3)
    pix, ix = QI.PqIndex(cb, codes), G.GipIndex(cv, ci)
    pqs, ixs = [], []
    try:
        s1, r1 = pix.search(qv, min(k1, n), out_device=True)
        us, ur = D.rerank_topk(ix, qv, qi, r1, k)
        assert bool((ur[:, : min(k, n)] >= 0).all())
        for r in range(ns):
            lo, hi = D.shard_bounds(n, ns, r)
            pqs.append(QI.PqIndex(cb, QI.encode(cv[lo:hi], cb), row_offset=lo))
            assert torch.equal(QI.encode(cv[lo:hi], cb), codes[lo:hi])               # a shard's codes are its slice of the corpus' codes
            ixs.append(G.GipIndex(cv[lo:hi], ci[lo:hi], row_offset=lo))
        ss, sr = D.pq_sharded_search(pqs, ixs, qv, qi, k1, k)
        assert torch.equal(sr, ur), "rows differ for queries %s" % torch.nonzero((sr != ur).any(dim=1)).flatten()[:8].tolist()
        assert torch.equal(ss.view(torch.int32), us.view(torch.int32))
    finally:
        for h in pqs + ixs + [pix, ix]:
            h.close()


def test_gated_image_default_by_size(G, monkeypatch):
    """DHR_OPT_GATED_I8 = -1 (the library's default): a small shard keeps the fp16 image of the gated columns (below 1 M rows the extra
    candidates of the looser int8 bound cost more than its cheaper GEMM saves); 0 / 1 force it.  Results are identical either way."""
    from dhr_amd import _lib, synth
    cv, ci, qv, qi = synth.make_pair(61, 20_000, 8, 768, 128)
    q32 = qv.astype(np.float32)
    out = {}
    for setting in ("-1", "0", "1"):
        monkeypatch.setenv("DHR_GATED_I8", setting)
        ix = G.GipIndex(cv, ci)
        try:
            assert ix.info(_lib.INFO_GATED_I8) == (1 if setting == "1" else 0)
            out[setting] = ix.search(q32, qi, 100)
        finally:
            ix.close()
    for setting in ("0", "1"):
        np.testing.assert_array_equal(out[setting][1], out["-1"][1])
        np.testing.assert_array_equal(out[setting][0], out["-1"][0])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["gauss", "outlier_columns", "spiky_rows", "tiny", "fp32_queries", "one_hot_queries"])
def test_dense_only_residual_refine(G, kind):
    """Dense-only int8 index (`dhr_set_option(DHR_OPT_DENSE_I8, 1)`): between the filter and the exact rescoring sits the RESIDUAL level --
    768 bytes per candidate that hold what the int8 image lost (in 1/254 of a column's step), so that the corpus half of the margin is
    measured instead of bounded.  Results equal the fp16 index's bit for bit and the oracle's top-k on inputs that stress both roundings;
    on plain Gaussian columns the level removes most of the bound candidates."""
    from dhr_amd import _lib
    rng = np.random.default_rng(zlib.crc32(kind.encode()) % 997)
    n, nq, d, k = 60_000, 24, 768, 100
    cv = (rng.standard_normal((n, d)) * 0.1).astype(np.float32)
    qv = (rng.standard_normal((nq, d)) * 0.1).astype(np.float32)
    if kind == "outlier_columns":
        cv[:, ::97] *= 30.0
        qv[:, ::97] *= 0.2
    elif kind == "spiky_rows":
        cv[::11] = 0
        cv[np.arange(0, n, 11), rng.integers(0, d, len(range(0, n, 11)))] = 6.0
    elif kind == "tiny":
        cv *= 1e-3
    elif kind == "fp32_queries":
        qv = qv * np.float32(1.0001) + np.float32(1e-5)
    elif kind == "one_hot_queries":
        qv[:] = 0
        qv[np.arange(nq), rng.integers(0, d, nq)] = 1.5
    cv = cv.astype(np.float16)
    qv = qv.astype(np.float32)
    st0, st1, _, _ = _i8_pair(G, cv, None, qv, None, k)
    if kind == "gauss":
        assert st1["candidates_exact"] - 64 * nq < 0.6 * st1["candidates_bound"], st1      # the residual level did prune (`exact` also counts the <= 64 bootstrap rows of every query)
