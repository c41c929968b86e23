"""Streamed exact inner-product search over fp32 vectors of any width, on `dhr_stream_search_*` (csrc/stream_search.hip): the reference's second
retrieval route, "no densification before retrieval" (`tevatron/datasets/beir/encode_and_retrieval.py`), where every text is one fp32 row
[lexical reps over the whole vocabulary | semantic reps] and the corpus is scored chunk by chunk against a running top-k per query.

    s = StreamSearch(q_lex, q_sem, k=1000)          # or StreamSearch(q) for one concatenated matrix
    for p_lex, p_sem in chunks: s.add(p_lex, p_sem)
    scores, rows = s.result()                       # [Q, k] fp32, [Q, k] int64; (-inf, -1) beyond the rows seen

The two column segments are passed as they are, with their row strides: no [n, V + d] concatenation is made.  Arrays are 2-D numpy arrays (host
memory: staged through the device block by block, the call is complete on return) or torch CUDA tensors (read in place; the call is enqueued on
torch's current stream and does not wait).  Values are read as fp32; any other dtype is converted once.  A score is a function of its two rows
alone, bit for bit, whatever the chunking, the order of the `add` calls or `block_rows`; its error is at most 2^-15 sum |q_c p_c|
(tests/test_stream_search.py).  Equal scores are listed in increasing row order.  There is no CPU implementation: without the HIP library / a GPU
the calls raise."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import _marshal as M

MAX_D, MAX_Q, MAX_K, ROW_TILE, MAX_BLOCK = 131072, 65536, 4096, 128, 65536


def _segment(a, what):
    """-> the fp32 operand the library reads in place (or one packed copy), its row stride"""
    if len(a.shape) != 2:
        raise ValueError("{} must be 2-D [n, d], got shape {}".format(what, tuple(a.shape)))
    if not M.is_np(a) and not a.is_cuda:
        a = a.detach().numpy()
    a, ld = M.as_read(M.cast(a, "float32"))
    return a, ld[0]


def _pair(a, b, what):
    """the two segments of a call: where they live, their sizes -> (a, ld_a, b or None, ld_b)"""
    a, ld_a = _segment(a, what + "_a")
    if b is not None and int(b.shape[-1]) == 0:
        b = None
    if b is None:
        return a, ld_a, None, 0
    b, ld_b = _segment(b, what + "_b")
    if M.is_np(a) != M.is_np(b) or (not M.is_np(a) and a.device != b.device):
        raise ValueError("{}_a and {}_b must live in the same memory".format(what, what))
    if int(a.shape[0]) != int(b.shape[0]):
        raise ValueError("{}_a has {} rows, {}_b has {}".format(what, int(a.shape[0]), what, int(b.shape[0])))
    return a, ld_a, b, ld_b


class StreamSearch:
    """The running top-k of every query over the passages added so far.  q_a [Q, d_a] and q_b [Q, d_b] (or None) are the queries' two column
    segments; block_rows is the number of passage rows scored between two selects (0: the library's default; else a multiple of 128 in
    [128, 65536])."""

    def __init__(self, q_a, q_b=None, k=1000, block_rows=0):
        self._h, self._last = None, None
        a, ld_a, b, ld_b = _pair(q_a, q_b, "q")
        self.n_queries, self.d_a, self.d_b = int(a.shape[0]), int(a.shape[1]), 0 if b is None else int(b.shape[1])
        self.k, self.block_rows, self.rows_added = int(k), int(block_rows), 0
        if not 1 <= self.n_queries <= MAX_Q:
            raise ValueError("between 1 and {} queries, got {}".format(MAX_Q, self.n_queries))
        if self.d_a < 1 or self.d_a + self.d_b > MAX_D:
            raise ValueError("between 1 and {} columns, got {} + {}".format(MAX_D, self.d_a, self.d_b))
        if not 1 <= self.k <= MAX_K:
            raise ValueError("k must be in [1, {}], got {}".format(MAX_K, self.k))
        if self.block_rows and (self.block_rows % ROW_TILE or not ROW_TILE <= self.block_rows <= MAX_BLOCK):
            raise ValueError("block_rows must be 0 or a multiple of {} in [{}, {}], got {}".format(ROW_TILE, ROW_TILE, MAX_BLOCK, self.block_rows))
        self._device = M.device(a)
        self._lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self._lib.dhr_stream_search_create(self._device, M.mem_kind(a), M.data_ptr(a), ld_a, M.data_ptr(b), ld_b, _lib.VAL_F32, self.n_queries,
                                                      self.d_a, self.d_b, self.k, self.block_rows, C.byref(h), M.stream(a)), "dhr_stream_search_create")
        self._h = h
        self._like = a if not M.is_np(a) else None      # results live where the queries live
        self._keep = (a, b)                             # the split is enqueued: the queries stay alive behind it

    def add(self, p_a, p_b=None, row_base=None):
        """Scores the passages p_a [n, d_a] (and p_b [n, d_b]) against every query and merges them into the lists; their rows are reported as
        row_base + position (None: they continue after the rows added so far).  Returns self."""
        if self._h is None:
            raise ValueError("the search is closed")
        a, ld_a, b, ld_b = _pair(p_a, p_b, "p")
        n, d_a, d_b = int(a.shape[0]), int(a.shape[1]), 0 if b is None else int(b.shape[1])
        if (d_a, d_b) != (self.d_a, self.d_b):
            raise ValueError("passages of {} + {} columns against queries of {} + {}".format(d_a, d_b, self.d_a, self.d_b))
        if not M.is_np(a) and M.device(a) != self._device:
            raise ValueError("passages on cuda:{}, the search is on cuda:{}".format(M.device(a), self._device))
        base = self.rows_added if row_base is None else int(row_base)
        if base < 0:
            raise ValueError("row_base must be >= 0, got {}".format(base))
        _lib.check(self._lib.dhr_stream_search_add(self._h, M.mem_kind(a), M.data_ptr(a), ld_a, M.data_ptr(b), ld_b, _lib.VAL_F32, n, base, self._stream(a)),
                   "dhr_stream_search_add")
        if not M.is_np(a):
            import torch
            for t in (a, b):                            # a converted or packed copy must outlive the kernels that read it
                if t is not None:
                    t.record_stream(torch.cuda.current_stream(t.device))
        self.rows_added = max(self.rows_added, base + n)
        return self

    def _stream(self, a=None):
        """the stream of a call: torch's current one where the call's arrays (else the queries) are CUDA tensors; for host arrays against host
        queries the stream of the latest call, so that the lists are read behind whatever wrote them"""
        if a is not None and not M.is_np(a):
            self._last = M.stream(a)
        elif self._like is not None:
            self._last = M.stream(self._like)
        return self._last

    def result(self):
        """-> (scores [Q, k] float32, rows [Q, k] int64): score descending, row ascending on exact ties, (-inf, -1) beyond the rows seen.  Torch
        tensors on the queries' device when the queries were one, else numpy arrays.  The search goes on."""
        if self._h is None:
            raise ValueError("the search is closed")
        like = self._like if self._like is not None else np.empty(0, np.float32)
        scores, rows = M.empty(like, (self.n_queries, self.k), "float32"), M.empty(like, (self.n_queries, self.k), "int64")
        _lib.check(self._lib.dhr_stream_search_result(self._h, M.data_ptr(scores), M.data_ptr(rows), M.mem_kind(like), self._stream()), "dhr_stream_search_result")
        return scores, rows

    def device_bytes(self):
        return int(self._lib.dhr_stream_search_device_bytes(self._h)) if self._h is not None else 0

    def close(self):
        if self._h is not None:
            self._lib.dhr_stream_search_destroy(self._h)
            self._h = None
            self._keep = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


def search(q, chunks, k=1000, block_rows=0):
    """The loop over an iterable: q is one matrix or a pair (q_a, q_b); every chunk is one matrix or a pair (p_a, p_b), numbered in the order
    they come -> (scores [Q, k], rows [Q, k])."""
    q_a, q_b = q if isinstance(q, (tuple, list)) else (q, None)
    with StreamSearch(q_a, q_b, k=k, block_rows=block_rows) as s:
        for chunk in chunks:
            p_a, p_b = chunk if isinstance(chunk, (tuple, list)) else (chunk, None)
            s.add(p_a, p_b)
        return s.result()
