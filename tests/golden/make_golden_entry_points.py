#!/usr/bin/env python
"""What the entry points of api.hip and pq_adc.hip COMPUTE and how they ANSWER bad arguments, pinned to the commit before their host code was
rewritten around one staging vocabulary and one error style.  Two recordings:

  tests/golden/entry_points.json        collect_checks(): every validation exit that is reached before the first HIP call -- (call, status, exact
                                        dhr_last_error text) -- and the two host merges on inputs full of ties.  No GPU needed.
  tests/golden/entry_points_gpu.json    collect(): dhr_search / dhr_search_rerank / dhr_score_rows / the debug hooks on a 1000-row index (fp16 and
                                        int8 gated image), dhr_densify, the PQ functions, the dhr_pq_* handle and the device merges, each from host
                                        and from device memory.  Only integers, hex representations of floats and SHA-256 digests of the output
                                        arrays are recorded, so tests/test_entry_points_golden.py compares for equality.

Run at the commit whose behaviour is to be pinned:   python tests/golden/make_golden_entry_points.py [--checks-only]
The GPU recording is made twice: a run that finds entry_points_gpu.json keeps only the fields that come out equal to the file's and lists what it
dropped under "_dropped" (ALLOWED_TO_DIFFER says what may stand there: pq_assign_kernel sums the training error with float atomics).

The bad-argument exits of dhr_debug_refine_bounds came with that hook: its null-handle exit in the first file, the exits behind the handle check (bad
range, null output, a range deeper than the candidate lists, a batch or an index without a refine level) as (status, error text) in the second.

The bad-argument exits of dhr_debug_select_merge came with that hook too, all in the first file: it takes no handle and refuses whatever its
kernels assume silently before it touches the device.

The index holds gated values that are integer multiples of 2^-6 (make_golden_index_build.py: the two-bucket deal of the default image is then the
same in every build), so the bound scores and the filter margins are pinned too."""
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATH_CHECKS = os.path.join(HERE, "entry_points.json")
PATH = os.path.join(HERE, "entry_points_gpu.json")

SEED, N, NQ, D_DLR, D_CLS, ROW_OFFSET, K, K1, M_ROWS = 9100, 1000, 5, 64, 64, 12345, 10, 37, 7      # 1000 rows do not fill four 256-row tiles
PQ_N, PQ_D, PQ_LD, PQ_M = 700, 32, 40, 4
ADC_N, ADC_K, ADC_K_REGROW = 40_000, 10, 100                                                         # more than one 16 384-row block
ALLOWED_TO_DIFFER = ("out_error",)           # of two recordings at one commit; timings and codebooks after iters >= 1 are not recorded at all
INVALID, UNSUPPORTED = -1, -2
HOST, DEVICE = 0, 1
F16, F32 = 0, 1
U8, I16 = 1, 3


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------ validation exits (CPU)
def _check_cases(lib, _lib):
    """-> {name: thunk}; a thunk makes one call that must fail before the library touches the device"""
    f16 = np.zeros((4, 64), np.float16)
    f32 = np.zeros((4, 64), np.float32)
    u8 = np.zeros((4, 64), np.uint8)
    out = np.zeros((4, 64), np.float32)
    p16, p32, pu8, pout = f16.ctypes.data, f32.ctypes.data, u8.ctypes.data, out.ctypes.data
    qb, _keep = _lib.make_query_batch(f32, None)
    qbp = C.byref(qb)
    bad_kind = _lib.QueryBatch()
    C.memmove(C.byref(bad_kind), qbp, C.sizeof(qb))
    bad_kind.mem_kind = 7
    err = C.c_double()
    handle = C.c_void_p()
    lo, un = C.c_int32(-5), C.c_int32(-5)
    keep = (f16, f32, u8, out, qb, bad_kind, _keep)

    def densify(mem_kind=HOST, lexical=p16, value_dtype=F16, ld=64, batch=4, vocab=64, remove_dims=0, dims=8, out_value=pout, out_dtype=F32, ld_value=8,
                out_index=pu8, index_dtype=U8, ld_index=8):
        return lambda: lib.dhr_densify(0, mem_kind, lexical, value_dtype, ld, batch, vocab, remove_dims, dims, out_value, out_dtype, ld_value, out_index, index_dtype,
                                       ld_index, None)

    def train(nbits=8, mem_kind=HOST, values=p16, ld=64, n=4, d=64, M=4, iters=1, max_points=256, codebooks=p32, plain=False):
        if plain:
            return lambda: lib.dhr_pq_train(0, mem_kind, values, ld, n, d, M, iters, max_points, codebooks, C.byref(err), None)
        return lambda: lib.dhr_pq_train_nbits(0, mem_kind, values, ld, n, d, M, nbits, iters, max_points, codebooks, C.byref(err), None)

    def encode(nbits=8, mem_kind=HOST, values=p16, ld=64, n=4, d=64, M=4, codebooks=p32, codes=pu8, plain=False):
        if plain:
            return lambda: lib.dhr_pq_encode(0, mem_kind, values, ld, n, d, M, codebooks, codes, None)
        return lambda: lib.dhr_pq_encode_nbits(0, mem_kind, values, ld, n, d, M, nbits, codebooks, codes, None)

    def decode(nbits=8, mem_kind=HOST, codes=pu8, n=4, d=64, M=4, codebooks=p32, out_values=p16, ld_out=64, plain=False):
        if plain:
            return lambda: lib.dhr_pq_decode(0, mem_kind, codes, n, d, M, codebooks, out_values, ld_out, None)
        return lambda: lib.dhr_pq_decode_nbits(0, mem_kind, codes, n, d, M, nbits, codebooks, out_values, ld_out, None)

    def create(mem_kind=HOST, n=4, d=64, M=4, nbits=8, codebooks=p32, codes=pu8, out_handle=True):
        return lambda: lib.dhr_pq_create(0, mem_kind, n, d, M, nbits, codebooks, codes, 0, C.byref(handle) if out_handle else None)

    def merge(nq=2, n_in=4, scores=p32, rows=pout, k=2, outs=pout, outr=pout, host=False):
        if host:
            return lambda: lib.dhr_merge_topk_host(nq, n_in, scores, rows, k, outs, outr)
        return lambda: lib.dhr_merge_topk(0, nq, n_in, scores, rows, k, outs, outr, None)

    def lists(nq=2, n_lists=2, list_len=2, scores=p32, rows=pout, k=2, outs=pout, outr=pout, host=False):
        if host:
            return lambda: lib.dhr_merge_topk_lists_host(nq, n_lists, list_len, scores, rows, k, outs, outr)
        return lambda: lib.dhr_merge_topk_lists(0, nq, n_lists, list_len, scores, rows, k, outs, outr, None)

    def select(nq=2, k=10, k_keep=0, kp=64, kps=64, sort_n=128, monotone=0, topk=pout, keys=pout, ld_keys=64, cnt=pout, count_all=0, cap=64, margin=p32,
               tau=p32, thr=pout):
        # (host pointers stand in for the device arrays: every case is refused before the device is touched)
        return lambda: lib.dhr_debug_select_merge(0, nq, k, k_keep, kp, kps, sort_n, monotone, topk, keys, ld_keys, cnt, count_all, cap, margin, tau, thr, None)

    def ranks(fn):
        def call():
            lo.value = un.value = -5
            r = fn(None, 10, C.byref(lo), C.byref(un))
            return [r, lo.value, un.value]
        return call

    cases = {
        # ---- dhr_densify, in the order of its checks
        "densify_null_lexical": densify(lexical=None),
        "densify_null_out_value": densify(out_value=None),
        "densify_null_out_index": densify(out_index=None),
        "densify_null_beats_mem_kind": densify(lexical=None, mem_kind=7),
        "densify_mem_kind": densify(mem_kind=7),
        "densify_mem_kind_beats_sizes": densify(mem_kind=7, batch=-1),
        "densify_batch_negative": densify(batch=-1),
        "densify_vocab_zero": densify(vocab=0),
        "densify_dims_zero": densify(dims=0),
        "densify_remove_negative": densify(remove_dims=-1),
        "densify_remove_all": densify(remove_dims=64),
        "densify_ld_small": densify(ld=63),
        "densify_ld_value_small": densify(ld_value=7),
        "densify_ld_index_small": densify(ld_index=7),
        "densify_sizes_beat_divisibility": densify(dims=7, ld_value=6),
        "densify_not_divisible": densify(dims=7, ld_value=7, ld_index=7),
        "densify_divisibility_beats_dtype": densify(dims=7, ld_value=7, ld_index=7, value_dtype=9),
        "densify_value_dtype": densify(value_dtype=9),
        "densify_value_dtype_bf16": densify(value_dtype=2),
        "densify_out_dtype": densify(out_dtype=9),
        "densify_value_dtype_beats_index_dtype": densify(value_dtype=9, index_dtype=0),
        "densify_index_dtype": densify(index_dtype=2),
        "densify_u8_over_256_groups": densify(ld=600, vocab=600, dims=2, ld_value=2, ld_index=2),
        "densify_index_dtype_beats_group_count": densify(ld=600, vocab=600, dims=2, ld_value=2, ld_index=2, index_dtype=2),
        "densify_over_32767_groups": densify(ld=40000, vocab=40000, dims=1, ld_value=1, ld_index=1, index_dtype=I16),
        "densify_u8_rule_beats_32767": densify(ld=40000, vocab=40000, dims=1, ld_value=1, ld_index=1),
        "densify_empty_batch_is_ok": densify(batch=0),
        "densify_group_count_beats_empty_batch": densify(batch=0, ld=600, vocab=600, dims=2, ld_value=2, ld_index=2),
        # ---- pq_check, shared by the six PQ functions, then what each adds
        "pq_train_null_values": train(values=None),
        "pq_train_null_codebooks": train(codebooks=None),
        "pq_train_null_beats_mem_kind": train(values=None, mem_kind=7),
        "pq_train_mem_kind": train(mem_kind=7),
        "pq_train_mem_kind_beats_sizes": train(mem_kind=7, d=0),
        "pq_train_n_negative": train(n=-1),
        "pq_train_d_zero": train(d=0),
        "pq_train_m_zero": train(M=0),
        "pq_train_d_not_multiple": train(M=5),
        "pq_train_ld_small": train(ld=63),
        "pq_train_sizes_beat_width": train(d=130, M=2, ld=100),
        "pq_train_wide_subvectors": train(d=130, M=2, ld=130),
        "pq_train_width_beats_nbits": train(d=130, M=2, ld=130, nbits=9),
        "pq_train_nbits_zero": train(nbits=0),
        "pq_train_nbits_nine": train(nbits=9),
        "pq_train_nbits_beats_counts": train(nbits=9, n=0),
        "pq_train_n_zero": train(n=0),
        "pq_train_iters_negative": train(iters=-1),
        "pq_train_max_points_small": train(max_points=255),
        "pq_train_max_points_small_nbits5": train(nbits=5, max_points=31),
        "pq_train_plain_null": train(values=None, plain=True),
        "pq_train_plain_max_points_small": train(max_points=255, plain=True),
        "pq_encode_null_values": encode(values=None),
        "pq_encode_null_codebooks": encode(codebooks=None),
        "pq_encode_mem_kind": encode(mem_kind=7),
        "pq_encode_sizes": encode(M=5),
        "pq_encode_wide_subvectors": encode(d=130, M=2, ld=130),
        "pq_encode_nbits": encode(nbits=9),
        "pq_encode_nbits_beats_null_codes": encode(nbits=9, codes=None),
        "pq_encode_null_codes": encode(codes=None),
        "pq_encode_null_codes_beats_empty": encode(codes=None, n=0),
        "pq_encode_empty_is_ok": encode(n=0),
        "pq_encode_plain_null_codes": encode(codes=None, plain=True),
        "pq_decode_null_codes": decode(codes=None),
        "pq_decode_null_codebooks": decode(codebooks=None),
        "pq_decode_mem_kind": decode(mem_kind=7),
        "pq_decode_ld_out_small": decode(ld_out=63),
        "pq_decode_wide_subvectors": decode(d=130, M=2, ld_out=130),
        "pq_decode_nbits": decode(nbits=0),
        "pq_decode_nbits_beats_null_out": decode(nbits=0, out_values=None),
        "pq_decode_null_out": decode(out_values=None),
        "pq_decode_null_out_beats_empty": decode(out_values=None, n=0),
        "pq_decode_empty_is_ok": decode(n=0),
        "pq_decode_plain_null_out": decode(out_values=None, plain=True),
        # ---- dhr_pq_create and the null-handle exits of the handle's calls
        "pq_create_null_out": create(out_handle=False),
        "pq_create_null_codebooks": create(codebooks=None),
        "pq_create_null_codes": create(codes=None),
        "pq_create_n_zero": create(n=0),
        "pq_create_d_zero": create(d=0),
        "pq_create_m_zero": create(M=0),
        "pq_create_d_not_multiple": create(M=5),
        "pq_create_nbits_zero": create(nbits=0),
        "pq_create_nbits_nine": create(nbits=9),
        "pq_create_argument_beats_mem_kind": create(nbits=9, mem_kind=7),
        "pq_create_mem_kind": create(mem_kind=7),
        "pq_create_mem_kind_beats_lds": create(mem_kind=7, d=128, M=128),
        "pq_create_tables_exceed_lds": create(d=128, M=128),
        "pq_search_null_handle": lambda: lib.dhr_pq_search(None, qbp, 10, pout, pout, HOST, None),
        "pq_search_null_handle_beats_k": lambda: lib.dhr_pq_search(None, qbp, 0, pout, pout, HOST, None),
        "pq_adc_scores_null_handle": lambda: lib.dhr_pq_adc_scores(None, qbp, 0, 1, pout, None),
        "pq_last_scan_null_handle": lambda: lib.dhr_pq_last_scan(None, None, None),
        "pq_device_bytes_null_handle": lambda: [lib.dhr_pq_device_bytes(None)],
        # ---- shard reduce
        "merge_nq_zero": merge(nq=0),
        "merge_n_in_zero": merge(n_in=0),
        "merge_k_zero": merge(k=0),
        "merge_null_scores": merge(scores=None),
        "merge_null_rows": merge(rows=None),
        "merge_null_out_scores": merge(outs=None),
        "merge_null_out_rows": merge(outr=None),
        "merge_host_nq_zero": merge(nq=0, host=True),
        "merge_host_null_rows": merge(rows=None, host=True),
        "merge_host_null_out_rows": merge(outr=None, host=True),
        "merge_host_k_zero": merge(k=0, host=True),
        "lists_nq_zero": lists(nq=0),
        "lists_n_lists_zero": lists(n_lists=0),
        "lists_list_len_zero": lists(list_len=0),
        "lists_k_zero": lists(k=0),
        "lists_null_scores": lists(scores=None),
        "lists_null_out_scores": lists(outs=None),
        "lists_rows_without_out_rows": lists(outr=None),
        "lists_argument_beats_lds": lists(outr=None, n_lists=65),
        "lists_over_64": lists(n_lists=65, list_len=1),
        "lists_exceed_lds_with_rows": lists(n_lists=64, list_len=214, k=20),        # (13 696 + 20) * 12 B > 160 KiB
        "lists_exceed_lds_scores_only": lists(n_lists=64, list_len=640, k=10, rows=None, outr=None),
        "lists_host_nq_zero": lists(nq=0, host=True),
        "lists_host_null_scores": lists(scores=None, host=True),
        "lists_host_rows_without_out_rows": lists(outr=None, host=True),
        # ---- the staged calls and the rank queries without a handle
        "search_mid_null_handle": lambda: lib.dhr_search_mid(None, pout, 1, pout, None),
        "search_begin_rest_null_handle": lambda: lib.dhr_search_begin_rest(None, pout, pout, None),
        "search_finish_null_handle": lambda: lib.dhr_search_finish(None, pout, pout, pout, pout, DEVICE, None),
        "search_finish_null_handle_beats_null_outputs": lambda: lib.dhr_search_finish(None, None, None, None, None, 7, None),
        "search_begin_null_handle": lambda: lib.dhr_search_begin(None, qbp, 10, pout, None),
        "search_pre_null_handle": lambda: lib.dhr_search_pre(None, qbp, 10, 1, pout, None),
        "search_null_handle": lambda: lib.dhr_search(None, qbp, 10, pout, pout, HOST, None),
        "search_rerank_null_handle": lambda: lib.dhr_search_rerank(None, qbp, qbp, 20, 10, pout, pout, HOST, None),
        "score_rows_null_handle": lambda: lib.dhr_score_rows(None, qbp, 1, pout, pout, HOST, None),
        "debug_bound_scores_null_handle": lambda: lib.dhr_debug_bound_scores(None, qbp, 0, 1, pout, None),
        "debug_query_margins_null_handle": lambda: lib.dhr_debug_query_margins(None, qbp, pout, None),
        "debug_refine_bounds_null_handle": lambda: lib.dhr_debug_refine_bounds(None, qbp, 0, 1, None, 0, pout, pout, None, None, None),
        # ---- dhr_debug_select_merge, in the order of its checks (no handle: everything the kernels assume silently is refused up front)
        "select_merge_null_list": select(topk=None),
        "select_merge_null_keys": select(keys=None),
        "select_merge_null_margin": select(margin=None),
        "select_merge_null_tau": select(tau=None),
        "select_merge_null_thr": select(thr=None),
        "select_merge_null_beats_n_queries": select(thr=None, nq=0),
        "select_merge_n_queries_zero": select(nq=0),
        "select_merge_n_queries_beats_kp": select(nq=-1, kp=100),
        "select_merge_kp_not_a_power_of_two": select(kp=96),
        "select_merge_kp_below_64": select(kp=32, kps=32, sort_n=128),
        "select_merge_kp_above_2_20": select(kp=1 << 21, kps=64),
        "select_merge_kp_beats_kps": select(kp=96, kps=96),
        "select_merge_kps_not_a_power_of_two": select(kp=1024, kps=96, sort_n=2048),
        "select_merge_kps_below_64": select(kp=1024, kps=32, sort_n=2048),
        "select_merge_kps_above_kp": select(kp=64, kps=128, sort_n=256),
        "select_merge_k_zero": select(k=0),
        "select_merge_k_above_k_keep": select(k=10, k_keep=9),
        "select_merge_k_keep_negative": select(k=10, k_keep=-1),
        "select_merge_k_keep_above_kps": select(k=10, k_keep=129, kp=1024, kps=128, sort_n=2048),
        "select_merge_k_above_kps_without_k_keep": select(k=65, kp=128, kps=64, sort_n=256),
        "select_merge_rank_beats_sort_n": select(k=0, sort_n=64),
        "select_merge_sort_n_leaves_under_64": select(kp=64, kps=64, sort_n=127),
        "select_merge_sort_n_beyond_the_lds": select(k=10, kp=4096, kps=4096, sort_n=5 * 4096, ld_keys=64),
        "select_merge_sort_n_beats_ld_keys": select(sort_n=64, ld_keys=-1),
        "select_merge_ld_keys_negative": select(ld_keys=-1, cap=0),
        "select_merge_count_all_above_ld_keys": select(cnt=None, count_all=65),
        "select_merge_count_all_beats_cap": select(cnt=None, count_all=65, cap=65),
        "select_merge_cap_above_ld_keys": select(cap=65),
        "select_merge_cap_above_ld_keys_without_cnt": select(cnt=None, count_all=64, cap=65),
        "select_merge_too_many_queries_for_the_global_path": select(nq=65536, kp=32768, kps=32768),
        "debug_gemm_time_null_handle": lambda: lib.dhr_debug_gemm_time(None, qbp, 1, C.byref(err), None, None),
        "sample_rank_null_handle": lambda: [lib.dhr_search_sample_rank(None, 10)],
        "union_rank_null_handle": lambda: [lib.dhr_search_union_rank(None, 10)],
        "mid_ranks_null_handle": ranks(lib.dhr_search_mid_ranks),
        "pre_ranks_null_handle": ranks(lib.dhr_search_pre_ranks),
    }
    for name in ("async_mid", "async_pre", "async_begin_rest", "async_begin", "async_finish"):        # the enqueue-only forms (not in the binding's table)
        fn = getattr(lib, "dhr_internal_search_" + name[6:] + "_async")
        fn.restype = C.c_int
        args = {"async_mid": (None, pout, 1, pout, None), "async_pre": (None, qbp, 10, 1, pout, None), "async_begin_rest": (None, pout, pout, None),
                "async_begin": (None, qbp, 10, pout, None), "async_finish": (None, pout, pout, pout, pout, DEVICE, None)}[name]
        types = {"async_mid": [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p], "async_pre": [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p],
                 "async_begin_rest": [C.c_void_p] * 4, "async_begin": [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p],
                 "async_finish": [C.c_void_p] * 5 + [C.c_int32, C.c_void_p]}[name]
        fn.argtypes = types
        cases["search_" + name + "_null_handle"] = (lambda fn=fn, args=args: fn(*args))
    return cases, keep


def _host_merges(lib):
    """the two host merges on inputs full of ties (scores from a set of 7, -1 holes, +-0, a NaN): digests of what they return.  dhr_merge_topk_host
    gets rows that are distinct within a query (+0 and -0 share a score key, so two such entries of ONE row would tie under its rules and
    their order would be the sort's matter); dhr_merge_topk_lists_host, which breaks ties by position, gets repeated rows too."""
    rng = np.random.default_rng(77)
    pool = np.array([0.0, -0.0, 1.5, -2.25, 3.0, 1.5, np.inf], np.float32)
    out = {}
    nq, n_in = 3, 100
    s = pool[rng.integers(0, len(pool), (nq, n_in))]
    s[1, 17] = np.nan
    r = rng.integers(-1, 20, (nq, n_in)).astype(np.int64)
    distinct = np.stack([rng.permutation(n_in) for _ in range(nq)]).astype(np.int64)
    distinct[r < 0] = -1
    for k in (10, 120):
        os_, or_ = np.full((nq, k), 9.0, np.float32), np.full((nq, k), 9, np.int64)
        rc = lib.dhr_merge_topk_host(nq, n_in, s.ctypes.data, distinct.ctypes.data, k, os_.ctypes.data, or_.ctypes.data)
        out["merge_host_k%d" % k] = [rc, _digest(os_), _digest(or_)]
    n_lists, list_len = 4, 25
    sl = np.ascontiguousarray(s.reshape(nq, n_lists, list_len).transpose(1, 0, 2))          # [list][query][position]
    rl = np.ascontiguousarray(r.reshape(nq, n_lists, list_len).transpose(1, 0, 2))
    for k in (10, 120):
        for with_rows in (1, 0):
            os_, or_ = np.full((nq, k), 9.0, np.float32), np.full((nq, k), 9, np.int64)
            rc = lib.dhr_merge_topk_lists_host(nq, n_lists, list_len, sl.ctypes.data, rl.ctypes.data if with_rows else None, k, os_.ctypes.data,
                                               or_.ctypes.data if with_rows else None)
            out["lists_host_k%d_rows%d" % (k, with_rows)] = [rc, _digest(os_), _digest(or_)]
    return out


def collect_checks():
    """-> {"exits": {name: [status, last error text]} (or the values a rank query returns), "host_merges": {...}}"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from dhr_amd import _lib
    lib = _lib.load()
    cases, keep = _check_cases(lib, _lib)
    exits = {}
    for name, call in cases.items():
        lib.dhr_merge_topk_host(0, 0, None, None, 0, None, None)          # a known error record in front of every case: one that succeeds leaves it
        got = call()
        exits[name] = got if isinstance(got, list) else [int(got), lib.dhr_last_error().decode()]
    del keep
    return {"exits": exits, "host_merges": _host_merges(lib)}


# ------------------------------------------------------------------------------------------------ what the entry points compute (GPU)
@contextlib.contextmanager
def _gated_i8(on):
    before = os.environ.get("DHR_GATED_I8")
    os.environ["DHR_GATED_I8"] = str(on)
    try:
        yield
    finally:
        if before is None:
            del os.environ["DHR_GATED_I8"]
        else:
            os.environ["DHR_GATED_I8"] = before


def _search_corpus():
    from dhr_amd import synth
    cv, ci, qv, qi = synth.make_pair(SEED, N, NQ, D_DLR, D_CLS)
    g = np.round(cv[:, :D_DLR].astype(np.float32) * 64.0) / 64.0          # see the module docstring
    assert np.abs(g).sum(axis=0).max() < 2.0 ** 17
    cv = cv.copy()
    cv[:, :D_DLR] = g.astype(np.float16)
    return cv, ci, qv.astype(np.float32), qi


def _outputs(torch, kind, nq, k):
    """(scores, rows, their pointers, a function that returns both as numpy) in host or device memory, pre-filled"""
    if kind == DEVICE:
        s = torch.full((nq, k), 9.0, dtype=torch.float32, device="cuda")
        r = torch.full((nq, k), 9, dtype=torch.int64, device="cuda")
        return s.data_ptr(), r.data_ptr(), lambda: (s.cpu().numpy(), r.cpu().numpy())
    s, r = np.full((nq, k), 9.0, np.float32), np.full((nq, k), 9, np.int64)
    return s.ctypes.data, r.ctypes.data, lambda: (s, r)


def collect_search(G, _lib, torch):
    cv, ci, qv, qi = _search_corpus()
    lib = _lib.load()
    rng = np.random.default_rng(SEED)
    rows = rng.integers(ROW_OFFSET, ROW_OFFSET + N, (NQ, M_ROWS)).astype(np.int64)
    rows[:, 0], rows[:, -1] = ROW_OFFSET, ROW_OFFSET + N - 1                 # the first and the last row of the shard
    out = {}
    for image, on in (("gated_fp16", 0), ("gated_i8", 1)):
        rec = {}
        with _gated_i8(on):
            ix = G.GipIndex(cv, ci, row_offset=ROW_OFFSET)
        try:
            rec["info_GATED_I8"] = int(ix.info(_lib.INFO_GATED_I8))
            qb, keep = _lib.make_query_batch(qv, qi)
            qb_plain, keep_plain = _lib.make_query_batch(qv, None)

            def stats(tag):
                st = ix.stats()
                for f in ("n_rows", "n_queries", "k", "candidates_bound", "candidates_exact"):
                    rec[tag + "_stats_" + f] = int(st[f])

            def score_rows(tag):
                for kind, name in ((HOST, "host"), (DEVICE, "device")):
                    if kind == DEVICE:
                        tr = torch.from_numpy(rows).cuda()
                        ts = torch.full((NQ, M_ROWS), 9.0, dtype=torch.float32, device="cuda")
                        _lib.check(lib.dhr_score_rows(ix._h, C.byref(qb), M_ROWS, tr.data_ptr(), ts.data_ptr(), DEVICE, None), "dhr_score_rows")
                        got = ts.cpu().numpy()
                    else:
                        got = np.full((NQ, M_ROWS), 9.0, np.float32)
                        _lib.check(lib.dhr_score_rows(ix._h, C.byref(qb), M_ROWS, rows.ctypes.data, got.ctypes.data, HOST, None), "dhr_score_rows")
                    rec["%s_%s_sha256" % (tag, name)] = _digest(got)

            for kind, name in ((HOST, "host"), (DEVICE, "device")):
                ps, pr, get = _outputs(torch, kind, NQ, K)
                _lib.check(lib.dhr_search(ix._h, C.byref(qb), K, ps, pr, kind, None), "dhr_search")
                s, r = get()
                rec["search_%s_scores_sha256" % name], rec["search_%s_rows_sha256" % name] = _digest(s), _digest(r)
                stats("search_" + name)
                for stage1, qb1 in (("gated", qb), ("ungated", qb_plain)):
                    ps, pr, get = _outputs(torch, kind, NQ, K)
                    _lib.check(lib.dhr_search_rerank(ix._h, C.byref(qb1), C.byref(qb), K1, K, ps, pr, kind, None), "dhr_search_rerank")
                    s, r = get()
                    tag = "rerank_%s_%s" % (stage1, name)
                    rec[tag + "_scores_sha256"], rec[tag + "_rows_sha256"] = _digest(s), _digest(r)
                    stats(tag)
            score_rows("score_rows")
            ix.search(qv[:2], qi[:2], K)                                      # a smaller batch re-uses the workspace: 2 active queries
            score_rows("score_rows_after_smaller_batch")
            bound = torch.full((NQ, 100), 9.0, dtype=torch.float32, device="cuda")
            _lib.check(lib.dhr_debug_bound_scores(ix._h, C.byref(qb), 200, 300, bound.data_ptr(), None), "dhr_debug_bound_scores")      # rows of tiles 0 and 1
            rec["bound_scores_sha256"] = _digest(bound.cpu().numpy())
            margin = np.full(NQ, 9.0, np.float32)
            _lib.check(lib.dhr_debug_query_margins(ix._h, C.byref(qb), margin.ctypes.data, None), "dhr_debug_query_margins")
            rec["margins_sha256"] = _digest(margin)
            # dhr_debug_refine_bounds: the exits behind the handle check (what it computes: tests/test_refine_bounds.py)
            u, u2 = torch.full((NQ, N), 9.0, dtype=torch.float32, device="cuda"), torch.full((NQ, N), 9.0, dtype=torch.float32, device="cuda")

            def refine_exit(tag, h, batch, lo, hi, pu=u.data_ptr(), flat=0):
                lib.dhr_merge_topk_host(0, 0, None, None, 0, None, None)          # a known error record in front of the call (collect_checks)
                rec["refine_bounds_" + tag] = [int(lib.dhr_debug_refine_bounds(h, C.byref(batch), lo, hi, None, flat, pu, u2.data_ptr(), None, None, None)),
                                               lib.dhr_last_error().decode()]

            refine_exit("row_lo_negative", ix._h, qb, -1, 10)
            refine_exit("row_hi_beyond_the_shard", ix._h, qb, 0, N + 1)
            refine_exit("empty_range", ix._h, qb, 10, 10)
            refine_exit("null_output", ix._h, qb, 0, N, pu=None)
            refine_exit("flat_negative", ix._h, qb, 0, N, flat=-1)
            refine_exit("plain_ip_batch", ix._h, qb_plain, 0, N)                 # refined on the int8 image of the gated half only
            with _gated_i8(on):                                                  # 1536 rows against lists of 1024 entries
                deep = G.GipIndex(np.concatenate([cv, cv[:536]]), np.concatenate([ci, ci[:536]]))
            try:
                deep.set_param(_lib.PARAM_CAND_CAP, 1024)
                refine_exit("range_deeper_than_the_lists", deep._h, qb, 0, 1536)
                refine_exit("range_that_fits_the_lists", deep._h, qb, 512, 1536)
            finally:
                deep.close()
            dense = G.GipIndex(np.ascontiguousarray(cv[:, D_DLR:]), None)        # no gated columns, no residual image: no refine level
            try:
                qd = np.ascontiguousarray(qv[:, D_DLR:])
                qb_dense, keep_dense = _lib.make_query_batch(qd, None)
                refine_exit("index_without_a_refine_level", dense._h, qb_dense, 0, N)
            finally:
                dense.close()
            ms, flops = C.c_double(-1.0), C.c_double(-1.0)
            rec["gemm_time_status"] = int(lib.dhr_debug_gemm_time(ix._h, C.byref(qb), 1, C.byref(ms), C.byref(flops), None))
            rec["gemm_time_flops"] = float(flops.value).hex()
            rec["gemm_time_ms_positive"] = int(ms.value > 0.0)
            del keep, keep_plain
        finally:
            ix.close()
        out[image] = rec
    return out


def collect_densify(_lib, torch):
    lib = _lib.load()
    batch, remove, dims, groups = 3, 570, 8, 4
    vocab, ld, ld_value, ld_index = remove + groups * dims, remove + groups * dims + 6, dims + 3, dims + 5
    rng = np.random.default_rng(SEED + 1)
    lex = rng.standard_normal((batch, ld)).astype(np.float32)
    out = {}
    for vd, vname, vnp in ((F16, "f16", np.float16), (F32, "f32", np.float32)):
        for xd, xname, xnp in ((U8, "u8", np.uint8), (I16, "i16", np.int16)):
            for od, oname, onp in ((F16, "f16", np.float16), (F32, "f32", np.float32)):
                for kind, kname in ((HOST, "host"), (DEVICE, "device")):
                    src = lex.astype(vnp)
                    val, idx = np.full((batch, ld_value), 9, onp), np.full((batch, ld_index), 9, xnp)
                    if kind == DEVICE:
                        tsrc, tval, tidx = torch.from_numpy(src).cuda(), torch.from_numpy(val).cuda(), torch.from_numpy(idx).cuda()
                        ptrs = (tsrc.data_ptr(), tval.data_ptr(), tidx.data_ptr())
                    else:
                        ptrs = (src.ctypes.data, val.ctypes.data, idx.ctypes.data)
                    _lib.check(lib.dhr_densify(0, kind, ptrs[0], vd, ld, batch, vocab, remove, dims, ptrs[1], od, ld_value, ptrs[2], xd, ld_index, None), "dhr_densify")
                    if kind == DEVICE:
                        torch.cuda.synchronize()
                        val, idx = tval.cpu().numpy(), tidx.cpu().numpy()
                    out["in_%s_idx_%s_out_%s_%s" % (vname, xname, oname, kname)] = {"value_sha256": _digest(val), "index_sha256": _digest(idx)}
    return out


def collect_pq(_lib, torch):
    lib = _lib.load()
    rng = np.random.default_rng(SEED + 2)
    values = np.zeros((PQ_N, PQ_LD), np.float16)
    values[:, :PQ_D] = (rng.standard_normal((PQ_N, PQ_D)) * 0.5).astype(np.float16)
    values[:, PQ_D:] = 77.0                                                   # the padding of a row is never read
    out = {}
    for nbits in (8, 5):
        ksub, dsub = 1 << nbits, PQ_D // PQ_M
        fixed = (rng.standard_normal((PQ_M, ksub, dsub)) * 0.5).astype(np.float32)
        codes_in = rng.integers(0, ksub, (PQ_N, PQ_M)).astype(np.uint8)
        for kind, kname in ((HOST, "host"), (DEVICE, "device")):
            rec = {}
            cb = np.full((PQ_M, ksub, dsub), 9.0, np.float32)
            codes = np.full((PQ_N, PQ_M), 9, np.uint8)
            decoded = np.full((PQ_N, PQ_LD), 9.0, np.float16)
            err = C.c_double(-1.0)
            if kind == DEVICE:
                t = {n: torch.from_numpy(a).cuda() for n, a in (("values", values), ("cb", cb), ("fixed", fixed), ("codes", codes), ("codes_in", codes_in), ("decoded", decoded))}
                p = {n: a.data_ptr() for n, a in t.items()}
            else:
                p = {n: a.ctypes.data for n, a in (("values", values), ("cb", cb), ("fixed", fixed), ("codes", codes), ("codes_in", codes_in), ("decoded", decoded))}
            # max_points 300 of 700 rows: every second row trains; iters 0: the codebooks are the initial ones
            _lib.check(lib.dhr_pq_train_nbits(0, kind, p["values"], PQ_LD, PQ_N, PQ_D, PQ_M, nbits, 0, 300, p["cb"], C.byref(err), None), "dhr_pq_train_nbits")
            _lib.check(lib.dhr_pq_encode_nbits(0, kind, p["values"], PQ_LD, PQ_N, PQ_D, PQ_M, nbits, p["fixed"], p["codes"], None), "dhr_pq_encode_nbits")
            _lib.check(lib.dhr_pq_decode_nbits(0, kind, p["codes_in"], PQ_N, PQ_D, PQ_M, nbits, p["fixed"], p["decoded"], PQ_LD, None), "dhr_pq_decode_nbits")
            if kind == DEVICE:
                cb, codes, decoded = t["cb"].cpu().numpy(), t["codes"].cpu().numpy(), t["decoded"].cpu().numpy()
            rec["codebooks_iters0_sha256"], rec["codes_sha256"], rec["decoded_sha256"] = _digest(cb), _digest(codes), _digest(decoded)
            rec["out_error"] = float(err.value).hex()
            if nbits == 8:                                                    # the forms without nbits are the nbits = 8 ones
                cb2, codes2, dec2 = np.full_like(cb, 9.0), np.full_like(codes, 9), np.full_like(decoded, 9.0)
                hv = values
                _lib.check(lib.dhr_pq_train(0, HOST, hv.ctypes.data, PQ_LD, PQ_N, PQ_D, PQ_M, 0, 300, cb2.ctypes.data, None, None), "dhr_pq_train")
                _lib.check(lib.dhr_pq_encode(0, HOST, hv.ctypes.data, PQ_LD, PQ_N, PQ_D, PQ_M, fixed.ctypes.data, codes2.ctypes.data, None), "dhr_pq_encode")
                _lib.check(lib.dhr_pq_decode(0, HOST, codes_in.ctypes.data, PQ_N, PQ_D, PQ_M, fixed.ctypes.data, dec2.ctypes.data, PQ_LD, None), "dhr_pq_decode")
                rec["plain_forms_equal"] = int(_digest(cb2) == rec["codebooks_iters0_sha256"] and _digest(codes2) == rec["codes_sha256"] and _digest(dec2) == rec["decoded_sha256"])
            out["nbits%d_%s" % (nbits, kname)] = rec
    return out


def collect_pq_handle(_lib, torch):
    lib = _lib.load()
    rng = np.random.default_rng(SEED + 3)
    q = (rng.standard_normal((4, PQ_D)) * 0.5).astype(np.float32)
    out = {}
    for nbits in (8, 4):
        ksub, dsub = 1 << nbits, PQ_D // PQ_M
        cb = (rng.standard_normal((PQ_M, ksub, dsub)) * 0.5).astype(np.float32)
        codes = rng.integers(0, ksub, (ADC_N, PQ_M)).astype(np.uint8)
        for kind, kname in ((HOST, "host"), (DEVICE, "device")):
            rec = {}
            if kind == DEVICE:
                tcb, tcodes, tq = torch.from_numpy(cb).cuda(), torch.from_numpy(codes).cuda(), torch.from_numpy(q).cuda()
                torch.cuda.synchronize()
                pcb, pcodes = tcb.data_ptr(), tcodes.data_ptr()
            else:
                pcb, pcodes = cb.ctypes.data, codes.ctypes.data
            h = C.c_void_p()
            _lib.check(lib.dhr_pq_create(0, kind, ADC_N, PQ_D, PQ_M, nbits, pcb, pcodes, ROW_OFFSET, C.byref(h)), "dhr_pq_create")
            try:
                rec["created_device_bytes"] = int(lib.dhr_pq_device_bytes(h))
                for step, (nq, k) in (("q3_k10", (3, ADC_K)), ("q4_k10", (4, ADC_K)), ("q4_k100_regrown", (4, ADC_K_REGROW)), ("q3_k10_again", (3, ADC_K))):
                    qb, keep = _lib.make_query_batch(tq[:nq] if kind == DEVICE else q[:nq], None)
                    ps, pr, get = _outputs(torch, kind, nq, k)
                    _lib.check(lib.dhr_pq_search(h, C.byref(qb), k, ps, pr, kind, None), "dhr_pq_search")
                    s, r = get()
                    rec[step + "_scores_sha256"], rec[step + "_rows_sha256"] = _digest(s), _digest(r)
                    ms, code_bytes = C.c_double(-1.0), C.c_double(-1.0)
                    _lib.check(lib.dhr_pq_last_scan(h, C.byref(ms), C.byref(code_bytes)), "dhr_pq_last_scan")
                    rec[step + "_code_bytes"] = float(code_bytes.value).hex()
                    rec[step + "_device_bytes"] = int(lib.dhr_pq_device_bytes(h))
                    del keep
                qb, keep = _lib.make_query_batch(tq[:3] if kind == DEVICE else q[:3], None)
                adc = torch.full((3, 64), 9.0, dtype=torch.float32, device="cuda")
                _lib.check(lib.dhr_pq_adc_scores(h, C.byref(qb), 100, 164, adc.data_ptr(), None), "dhr_pq_adc_scores")
                rec["adc_scores_sha256"] = _digest(adc.cpu().numpy())
                rec["adc_scores_device_bytes"] = int(lib.dhr_pq_device_bytes(h))
                del keep
            finally:
                lib.dhr_pq_destroy(h)
            out["nbits%d_%s" % (nbits, kname)] = rec
    return out


def collect_merges(_lib, torch):
    lib = _lib.load()
    rng = np.random.default_rng(SEED + 4)
    nq, n_in, n_lists, list_len, k = 3, 100, 4, 25, 10
    pool = np.array([0.5, 1.5, -2.25, 3.0, 7.0, -0.0, 0.0], np.float32)
    s = pool[rng.integers(0, len(pool), (nq, n_in))] + rng.integers(0, 3, (nq, n_in)).astype(np.float32)
    r = rng.permutation(10 * nq * n_in)[:nq * n_in].reshape(nq, n_in).astype(np.int64)
    r[:, ::13] = -1
    sl = np.ascontiguousarray(-np.sort(-s.reshape(nq, n_lists, list_len), axis=2).transpose(1, 0, 2))       # [list][query][position], every list best first
    rl = np.ascontiguousarray(r.reshape(nq, n_lists, list_len).transpose(1, 0, 2))
    ts, tr, tsl, trl = (torch.from_numpy(a).cuda() for a in (s, r, sl, rl))
    out = {}
    os_ = torch.full((nq, k), 9.0, dtype=torch.float32, device="cuda")
    or_ = torch.full((nq, k), 9, dtype=torch.int64, device="cuda")
    _lib.check(lib.dhr_merge_topk(0, nq, n_in, ts.data_ptr(), tr.data_ptr(), k, os_.data_ptr(), or_.data_ptr(), None), "dhr_merge_topk")
    torch.cuda.synchronize()
    out["merge_topk"] = {"scores_sha256": _digest(os_.cpu().numpy()), "rows_sha256": _digest(or_.cpu().numpy())}
    for with_rows in (1, 0):
        os_.fill_(9.0)
        or_.fill_(9)
        _lib.check(lib.dhr_merge_topk_lists(0, nq, n_lists, list_len, tsl.data_ptr(), trl.data_ptr() if with_rows else None, k, os_.data_ptr(),
                                            or_.data_ptr() if with_rows else None, None), "dhr_merge_topk_lists")
        torch.cuda.synchronize()
        out["merge_topk_lists_rows%d" % with_rows] = {"scores_sha256": _digest(os_.cpu().numpy()), "rows_sha256": _digest(or_.cpu().numpy())}
    return out


def collect():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import torch
    from dhr_amd import _lib
    from dhr_amd.retrieval import gip_retrieval as G
    _lib.load()
    return {"search": collect_search(G, _lib, torch), "densify": collect_densify(_lib, torch), "pq": collect_pq(_lib, torch),
            "pq_handle": collect_pq_handle(_lib, torch), "merges": collect_merges(_lib, torch)}


def leaves(d, prefix=""):
    """{dotted path: value} of a nested dict"""
    out = {}
    for key, v in d.items():
        if isinstance(v, dict):
            out.update(leaves(v, prefix + key + "."))
        else:
            out[prefix + key] = v
    return out


def drop(d, paths, prefix=""):
    """d without the leaves named in paths"""
    return {key: drop(v, paths, prefix + key + ".") if isinstance(v, dict) else v for key, v in d.items() if prefix + key not in paths}


def _write(path, obj):
    with open(path, "w") as f:
        json.dump(obj, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


def main():
    _write(PATH_CHECKS, collect_checks())
    if "--checks-only" in sys.argv:
        return
    got = collect()
    dropped = []
    if os.path.exists(PATH):
        with open(PATH) as f:
            before = json.load(f)
        dropped = sorted(set(before.pop("_dropped", [])) | {p for p, v in leaves(got).items() if leaves(before).get(p, v) != v})
        print("fields that differ from the file (dropped):", dropped)
        got = drop(got, set(dropped))
    got["_dropped"] = dropped
    _write(PATH, got)


if __name__ == "__main__":
    main()
