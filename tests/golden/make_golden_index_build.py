#!/usr/bin/env python
"""What the index build PRODUCES, pinned to the commit before dhr_index_create was rewritten around one layout plan (index_layout.h): for a
set of small corpora that take every branch of the build -- every dhr_index_get_info id, the device bytes of the fresh handle, the bound
scores of ALL rows and the filter margins for a gated and an ungated batch of 16 queries (they read every device image the build writes:
operand tiles, column steps, row sums, bucket maps), and one serial search (scores, rows, candidate counts: the refine lists and the residual
image).  Only integers, hex representations of floats and SHA-256 digests are recorded, so tests/test_index_build_golden.py compares for
equality.

Needs the GPU.  Run at the commit whose behaviour is to be pinned:   python tests/golden/make_golden_index_build.py
A run that finds tests/golden/index_build.json keeps only the fields that come out equal to the file's and prints what it dropped: run it
twice.  tests/test_index_build_golden.py imports collect() from here.

The default image deals 8-bit index values to two buckets by a value-mass histogram that the build sums with floating-point atomics
(make_golden_controller_plan.py, IMAGES): the u8 two-bucket corpora here hold gated values that are integer multiples of 2^-6 with less than
2^17 of mass per slice, so every partial sum of the histogram is exact in fp32 whatever the order, and the deal is the same in every build."""
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATH = os.path.join(HERE, "index_build.json")

N, NQ, K = 2_900, 16, 50          # 11 whole tiles and a ragged one
TRIAL_ROWS, TRIAL_COLS, TRIAL_BLOCK = 1_000_000, 256, 4_096
INFO = ("DENSE_I8", "I8_SCALE", "I8_ROW_ERR", "I8_ROW_NORM", "ROW_NORM_MAX", "TILE_BYTES", "GATED_I8", "GEMM_KERNEL")
# name -> (corpus, DHR_DENSE_I8, DHR_GATED_I8, idx_buckets, source); -1 = the library's default
CASES = {
    "g64_gated_fp16": ("u8_64", -1, 0, 0, "host"),
    "g64_gated_i8": ("u8_64", -1, 1, 0, "host"),
    "g64_abs_gated_i8": ("u8_64_abs", -1, 1, 0, "host"),
    "pad100_host": ("u8_100", -1, -1, 0, "host"),
    "pad100_device": ("u8_100", -1, -1, 0, "device"),
    "pad100_file": ("u8_100", -1, -1, 0, "file"),
    "i16_value_mod_2": ("i16_64", -1, -1, 0, "host"),
    "one_bucket": ("u8_64", -1, -1, 1, "host"),
    "dense128_fp16": ("dense_128", 0, -1, 0, "host"),
    "dense128_i8_residual": ("dense_128", 1, -1, 0, "host"),
    "dense1100_i8_no_residual": ("dense_1100", 1, -1, 0, "host"),
    "trial_keeps_i8": ("trial_even", -1, -1, 0, "device"),
    "trial_falls_back": ("trial_spiky", -1, -1, 0, "device"),
}
SAME = ("pad100_host", "pad100_device", "pad100_file")      # one corpus from host memory, from device memory, through save + load


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _exact_mass(cv, d_dlr):
    """gated values -> integer multiples of 2^-6, every slice's mass below 2^17: the histogram's fp32 sums are exact in any order"""
    g = np.round(cv[:, :d_dlr].astype(np.float32) * 64.0) / 64.0
    assert np.abs(g).sum(axis=0).max() < 2.0 ** 17
    out = cv.copy()
    out[:, :d_dlr] = g.astype(np.float16)
    assert np.array_equal(out[:, :d_dlr].astype(np.float32), g)
    return out


def trial_ratio(block):
    """sqrt(d_cls) ec / nc of the build's int8 trial (index_build.hip, i8_row_err_kernel) for a dense-only block, in float64"""
    b = block.astype(np.float64)
    m = np.abs(b).max(axis=0)
    scale = m.max() / 127.0
    step = scale * np.maximum(np.where(m > 0, np.minimum(m / (127.0 * scale), 1.0), 1.0) ** 0.75, 1.0 / 1024.0)
    q8 = np.clip(np.rint(b / step), -127, 127)
    ec = np.sqrt((((b - step * q8) * (scale / step)) ** 2).sum(axis=1).max())
    nc = np.sqrt(((scale * q8) ** 2).sum(axis=1).max())
    return float(np.sqrt(b.shape[1]) * ec / nc)


def corpus(kind):
    """-> (corpus values fp16, corpus indices or None, query values fp32, query indices or None); the trial corpora as one block to tile"""
    from dhr_amd import synth
    rng = np.random.default_rng(4242)
    if kind in ("u8_64", "u8_64_abs", "u8_100"):
        d = 100 if kind == "u8_100" else 64
        cv, ci, qv, qi = synth.make_pair(8100 + d, N, NQ, d, 8)
        if kind == "u8_64_abs":
            cv[:, :d] *= np.where(rng.random((N, d)) < 0.3, -1, 1).astype(np.float16)
        return _exact_mass(cv, d), ci, qv.astype(np.float32), qi
    if kind == "i16_64":
        vocab = 64 * 3000       # whole-word vocabulary without background, as the bm25 corpora: index values up to 2999
        cv, ci = synth.make_dlr(rng, N, 64, 30, 90, vocab=vocab, background=False, idx_dtype=np.int16, perm=np.arange(vocab))
        qv, qi = synth.make_dlr(rng, NQ, 64, 4, 12, vocab=vocab, background=False, idx_dtype=np.int16, integer_weights=True, perm=np.arange(vocab))
        cv, qv = (np.concatenate([a, synth.make_dense(rng, a.shape[0], 8)], axis=1) for a in (cv, qv))
        assert ci.dtype == np.int16 and ci.max() > 255
        return cv, ci, qv.astype(np.float32), qi
    if kind in ("dense_128", "dense_1100"):
        cv, _, qv, _ = synth.make_pair(8400, N, NQ, 0, int(kind.split("_")[1]), kind="dense")
        return cv, None, qv.astype(np.float32), None
    q = (rng.standard_normal((NQ, TRIAL_COLS)) * 0.1).astype(np.float32)
    if kind == "trial_even":        # evenly spread values: the rounding error is a small share of a row's norm
        block = rng.uniform(-1.0, 1.0, (TRIAL_BLOCK, TRIAL_COLS)).astype(np.float16)
        assert trial_ratio(block) < 0.35, trial_ratio(block)
    else:                           # one large entry per row (every column gets one: all steps are 1/127) among entries below half a step, which the int8 image loses
        block = rng.uniform(0.0025, 0.0035, (TRIAL_BLOCK, TRIAL_COLS)).astype(np.float16)
        block[np.arange(TRIAL_BLOCK), np.arange(TRIAL_BLOCK) % TRIAL_COLS] = 1.0
        assert trial_ratio(block) > 0.55, trial_ratio(block)
    return block, None, q, None


@contextlib.contextmanager
def _options(dense_i8, gated_i8):
    """the two image options of the build, through the environment (which beats the process options)"""
    before = {v: os.environ.get(v) for v in ("DHR_DENSE_I8", "DHR_GATED_I8")}
    os.environ["DHR_DENSE_I8"], os.environ["DHR_GATED_I8"] = str(dense_i8), str(gated_i8)
    try:
        yield
    finally:
        for v, old in before.items():
            if old is None:
                del os.environ[v]
            else:
                os.environ[v] = old


def _build(G, torch, cv, ci, buckets, source):
    if source == "host":
        return G.GipIndex(cv, ci, idx_buckets=buckets)
    tv = torch.from_numpy(cv).cuda()
    if cv.shape[0] == TRIAL_BLOCK:
        tv = tv.repeat((TRIAL_ROWS + TRIAL_BLOCK - 1) // TRIAL_BLOCK, 1)[:TRIAL_ROWS].contiguous()
    ti = None if ci is None else torch.from_numpy(ci).cuda()
    if source == "device":
        return G.GipIndex(tv, ti, idx_buckets=buckets)
    first = G.GipIndex(tv, ti, idx_buckets=buckets)
    with tempfile.TemporaryDirectory() as tmp:
        try:
            first.save(os.path.join(tmp, "index.dhr"))
        finally:
            first.close()
        return G.GipIndex.load(os.path.join(tmp, "index.dhr"))[0]


def collect_case(G, _lib, name):
    import torch
    kind, dense_i8, gated_i8, buckets, source = CASES[name]
    cv, ci, qv, qi = corpus(kind)
    with _options(dense_i8, gated_i8):
        ix = _build(G, torch, cv, ci, buckets, source)
    try:
        rec = {"info_" + what: float(ix.info(getattr(_lib, "INFO_" + what))).hex() for what in INFO}
        rec["info_TILE_BYTES"], rec["info_DENSE_I8"], rec["info_GATED_I8"] = (int(ix.info(getattr(_lib, "INFO_" + w))) for w in ("TILE_BYTES", "DENSE_I8", "GATED_I8"))
        rec["device_bytes"] = ix.device_bytes()
        n = ix.n_rows
        out = torch.zeros((NQ, n), dtype=torch.float32, device="cuda")
        margin = np.zeros(NQ, np.float32)
        for batch, index in (("gated", qi), ("ungated", None)):
            if batch == "gated" and ci is None:
                continue
            qb, keep = _lib.make_query_batch(qv, index)
            _lib.check(ix._lib.dhr_debug_bound_scores(ix._h, C.byref(qb), 0, n, out.data_ptr(), None), "dhr_debug_bound_scores")
            _lib.check(ix._lib.dhr_debug_query_margins(ix._h, C.byref(qb), margin.ctypes.data, None), "dhr_debug_query_margins")
            rec[batch + "_bound_sha256"] = _digest(out.cpu().numpy())
            rec[batch + "_margins_sha256"] = _digest(margin)
            del keep
        ix.set_param(_lib.PARAM_OVERLAP_AUX, 0)
        scores, rows = ix.search(qv, qi, K)
        st = ix.stats()
        rec["search_scores_sha256"], rec["search_rows_sha256"] = _digest(scores), _digest(rows)
        rec["candidates_bound"], rec["candidates_exact"] = int(st["candidates_bound"]), int(st["candidates_exact"])
        rec["abs_mode"] = int(bool(ci is not None and (cv[:, :ci.shape[1]] < 0).any()))
        # dense-only int8 indexes whose residual rows fit 512 bytes have a residual image; it is part of the device bytes
        rec["residual"] = int(ci is None and rec["info_DENSE_I8"] == 1 and (cv.shape[1] + 255) // 256 * 128 <= 512)
    finally:
        ix.close()
    return rec


def check_coverage(got):
    """the cases must take both sides of every branch of the build"""
    assert got["trial_keeps_i8"]["info_DENSE_I8"] == 1 and got["trial_falls_back"]["info_DENSE_I8"] == 0
    for field in ("info_GATED_I8", "abs_mode", "residual", "info_DENSE_I8"):
        assert {c[field] for c in got.values()} == {0, 1}, field
    assert got["g64_gated_fp16"]["info_GATED_I8"] == 0 and got["g64_gated_i8"]["info_GATED_I8"] == 1 and got["g64_abs_gated_i8"]["info_GATED_I8"] == 1
    n, resid = got["dense128_i8_residual"], got["dense1100_i8_no_residual"]
    assert n["residual"] == 1 and resid["residual"] == 0
    assert n["device_bytes"] == N * 128 * 2 + N * 128 + n["info_TILE_BYTES"] and resid["device_bytes"] == N * 1152 * 2 + resid["info_TILE_BYTES"]
    for other in SAME[1:]:
        assert got[other] == got[SAME[0]], (other, {f: (v, got[SAME[0]][f]) for f, v in got[other].items() if v != got[SAME[0]][f]})


def collect(names=None):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from dhr_amd import _lib
    from dhr_amd.retrieval import gip_retrieval as G
    _lib.load()
    return {name: collect_case(G, _lib, name) for name in (names or CASES)}


def keep_equal(a, b):
    """the fields of a that b holds with the same value (nested dicts)"""
    out = {}
    for key, va in a.items():
        if key not in b:
            continue
        if isinstance(va, dict):
            out[key] = keep_equal(va, b[key])
        elif va == b[key]:
            out[key] = va
    return out


def main():
    got = collect()
    check_coverage(got)
    if os.path.exists(PATH):
        with open(PATH) as f:
            before = json.load(f)
        kept = keep_equal(got, before)
        print("fields that differ from the file (dropped):", json.dumps({c: [f for f in got[c] if got[c][f] != kept.get(c, {}).get(f)] for c in got}))
        got = kept
    with open(PATH, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print(os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
