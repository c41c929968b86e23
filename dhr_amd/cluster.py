"""k-means over whole record vectors on the fused HIP ops `dhr_kmeans_assign`, `dhr_kmeans_update` and `dhr_kmeans` (csrc/kmeans.hip): the
clustering behind the query-cluster files of topic-aware sampling (`python -m dhr_amd.cluster_queries`).

`values` is a 2-D numpy array (host memory: staged through the device, complete on return) or a torch CUDA tensor (read in place: the op is
enqueued on torch's current stream and the call does not wait for it); the results live where the values live.  Rows are read as fp16, the
index record's dtype: any other dtype is converted once and never reinterpreted.  `columns=(lo, hi)` selects a column range of the records by
pointer offset, without a copy.  The nearest centroid is the one with the largest <x, c> - |c|^2 / 2, the lowest index on a tie; a cluster
without members keeps its centroid; nothing is summed with atomics, so two calls on the same arguments give the same bits.  There is no CPU
implementation: without the HIP library / a GPU the calls raise."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import _lib
from . import _marshal as M

MAX_D, MAX_K = 4096, 65536

KMeans = namedtuple("KMeans", "centroids assign counts objective changed")


def _f16_values(values):
    """fp16 rows as they are, everything else converted (quantize_index._f16_values)"""
    if M.is_np(values):
        return values if values.dtype == np.float16 else values.astype(np.float16)
    import torch
    return values if values.dtype == torch.float16 else values.half()


def _rows(values, columns):
    """-> (fp16 rows with a unit column stride, the column view the library reads, ld)"""
    if len(values.shape) != 2:
        raise ValueError("values must be 2-D [n, d], got shape {}".format(tuple(values.shape)))
    values = _f16_values(values)
    if not M.is_np(values) and not values.is_cuda:
        values = values.numpy()
    lo, hi = (0, int(values.shape[1])) if columns is None else (int(columns[0]), int(columns[1]))
    if not 0 <= lo < hi <= int(values.shape[1]):
        raise ValueError("columns {}:{} outside a record of {} columns".format(lo, hi, int(values.shape[1])))
    values, _ = M.as_read(values)
    view = values[:, lo:hi]
    if int(view.shape[0]) < 1:
        raise ValueError("values has no rows")
    if int(view.shape[1]) > MAX_D:
        raise ValueError("at most {} columns, got {}".format(MAX_D, int(view.shape[1])))
    return values, view, M.lds(values)[0]


def _like(view, a, dtype, shape, what):
    """`a` as a contiguous array of `dtype` where the rows live"""
    if tuple(a.shape) != tuple(shape):
        raise ValueError("{} must have shape {}, got {}".format(what, tuple(shape), tuple(a.shape)))
    if M.is_np(view):
        if not M.is_np(a):
            a = a.detach().cpu().numpy()
        return np.ascontiguousarray(a, dtype)
    import torch
    if M.is_np(a):
        a = torch.from_numpy(np.ascontiguousarray(a))
    return a.to(device=view.device, dtype=getattr(torch, dtype)).contiguous()


def assign(values, centroids, *, columns=None):
    """-> (assign int32 [n], dist float32 [n]): the nearest centroid of every row and |x - c|^2 to it.  centroids: fp32 [K, d]."""
    keep, view, ld = _rows(values, columns)
    n, d = int(view.shape[0]), int(view.shape[1])
    if len(centroids.shape) != 2:
        raise ValueError("centroids must be 2-D [K, d]")
    K = int(centroids.shape[0])
    c = _like(view, centroids, "float32", (K, d), "centroids")
    out_a, out_d = M.empty(view, (n,), "int32"), M.empty(view, (n,), "float32")
    lib = _lib.load()
    _lib.check(lib.dhr_kmeans_assign(M.device(view), M.mem_kind(view), M.data_ptr(view), ld, n, d, M.data_ptr(c), K, M.data_ptr(out_a), M.data_ptr(out_d),
                                     M.stream(view)), "dhr_kmeans_assign")
    del keep
    return out_a, out_d


def update(values, assign, centroids, *, columns=None):
    """-> (centroids float32 [K, d], counts int64 [K]): every centroid the fp32 mean of its members, added in increasing row order; a cluster
    without members keeps the centroid given.  `centroids` itself is not written."""
    keep, view, ld = _rows(values, columns)
    n, d = int(view.shape[0]), int(view.shape[1])
    if len(centroids.shape) != 2:
        raise ValueError("centroids must be 2-D [K, d]")
    K = int(centroids.shape[0])
    c = _like(view, centroids, "float32", (K, d), "centroids")
    if c is centroids or (not M.is_np(c) and c.data_ptr() == M.data_ptr(centroids)) or (M.is_np(c) and np.shares_memory(c, centroids)):
        c = c.copy() if M.is_np(c) else c.clone()
    a = _like(view, assign, "int32", (n,), "assign")
    counts = M.empty(view, (K,), "int64")
    lib = _lib.load()
    _lib.check(lib.dhr_kmeans_update(M.device(view), M.mem_kind(view), M.data_ptr(view), ld, n, d, M.data_ptr(a), K, M.data_ptr(c), M.data_ptr(counts),
                                     M.stream(view)), "dhr_kmeans_update")
    del keep
    return c, counts


def initial_rows(n: int, n_clusters: int, seed: int = 0):
    """the rows that seed the centroids when no `init` is given: the first n_clusters of a PCG64(seed) permutation of the rows, in that order"""
    if n_clusters > n:
        raise ValueError("{} clusters need an `init`: there are only {} rows to draw from".format(n_clusters, n))
    return np.random.Generator(np.random.PCG64(int(seed))).permutation(int(n))[:int(n_clusters)].astype(np.int64)


def kmeans(values, n_clusters, *, iters=20, seed=0, init=None, columns=None):
    """Exactly `iters` rounds of assign + update and one last assign -> KMeans(centroids float32 [K, d], assign int32 [n], counts int64 [K],
    objective float64 [iters + 1], changed int64 [iters + 1]); assign, counts and objective[-1] describe the centroids returned.
    init: int64 row positions [K] (the centroids start as those rows), an fp32 [K, d] array, or None: initial_rows(n, K, seed)."""
    keep, view, ld = _rows(values, columns)
    n, d = int(view.shape[0]), int(view.shape[1])
    K, iters = int(n_clusters), int(iters)
    if not 1 <= K <= MAX_K:
        raise ValueError("n_clusters must be in [1, {}], got {}".format(MAX_K, K))
    if iters < 0:
        raise ValueError("iters must be >= 0, got {}".format(iters))
    if init is None:
        init = initial_rows(n, K, seed)
    if len(init.shape) == 1:
        if "int" not in M.dtype_name(init) or int(init.shape[0]) != K:
            raise ValueError("init must be {} integer row positions or an fp32 [{}, {}] array".format(K, K, d))
        pos = np.asarray(init if M.is_np(init) else init.detach().cpu().numpy(), np.int64)
        if pos.min() < 0 or pos.max() >= n:
            raise ValueError("init names a row outside [0, {})".format(n))
        if M.is_np(view):
            c = np.ascontiguousarray(view[pos].astype(np.float32))
        else:
            import torch
            c = view[torch.from_numpy(pos).to(view.device)].float().contiguous()
    else:
        c = _like(view, init, "float32", (K, d), "init")
        if M.is_np(c) and np.shares_memory(c, init):
            c = c.copy()
        elif not M.is_np(c) and not M.is_np(init) and c.data_ptr() == init.data_ptr():
            c = c.clone()
    out_a, counts = M.empty(view, (n,), "int32"), M.empty(view, (K,), "int64")
    objective, changed = M.empty(view, (iters + 1,), "float64"), M.empty(view, (iters + 1,), "int64")
    lib = _lib.load()
    _lib.check(lib.dhr_kmeans(M.device(view), M.mem_kind(view), M.data_ptr(view), ld, n, d, K, iters, M.data_ptr(c), M.data_ptr(out_a), M.data_ptr(counts),
                              M.data_ptr(objective), M.data_ptr(changed), M.stream(view)), "dhr_kmeans")
    del keep
    return KMeans(c, out_a, counts, objective, changed)
