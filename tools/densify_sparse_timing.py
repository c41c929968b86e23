#!/usr/bin/env python
"""Times of the sparse densify (profiles/densify_sparse.txt).

    python tools/densify_sparse_timing.py [--vectors 100000 1000000] [--entries 60] [--dims 768]
        dhr_amd.densify_sparse.densify_vectors_into on device arrays: int32 ids over a 2 M term vocabulary (BM25, omission 472, int16 index),
        float32 weights, row lengths Poisson(entries).  Device events around each call, 3 warm-ups, median and fastest of 15; the bytes the op
        writes (dims * 4 per vector, 4 for its collision count) and reads (8 per entry, 8 per row pointer) per second.

    python tools/densify_sparse_timing.py --reference <root of the reference checkout> [--vectors 2000]
        the reference's `densify` (densify/densify_corpus.py, loaded by its path with pyserini.index stubbed) on the same kind of vectors as
        {term: weight} dicts, on this host's CPU, one process: seconds per 1 000 vectors."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def vectors(n, entries, vocab, seed=1):
    rng = np.random.default_rng(seed)
    lens = rng.poisson(entries, n)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(indptr[-1])
    return indptr, rng.integers(0, vocab, nnz).astype(np.int32), rng.uniform(0.05, 12.0, nnz).astype(np.float32)


def device(args):
    import torch
    from dhr_amd import densify_sparse as DS
    print(f"device: {torch.cuda.get_device_name(0)}; dims {args.dims}, int16 index, about {args.entries} entries per vector")
    for n in args.vectors:
        indptr, ids, w = (torch.from_numpy(a).cuda() for a in vectors(n, args.entries, 2_000_000))
        value = torch.empty((n, args.dims), dtype=torch.float16, device="cuda")
        index = torch.empty((n, args.dims), dtype=torch.int16, device="cuda")
        ms = []
        for it in range(18):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            DS.densify_vectors_into(indptr, ids, w, value, index, args.dims, 472)
            e1.record()
            torch.cuda.synchronize()
            if it >= 3:
                ms.append(e0.elapsed_time(e1))
        med, best = float(np.median(ms)), min(ms)
        written, read = n * (args.dims * 4 + 4), int(ids.numel()) * 8 + (n + 1) * 8
        print(f"vectors {n:>8}  entries {int(ids.numel()):>9}  median {med:8.3f} ms  fastest {best:8.3f} ms  written {written / med / 1e6:8.1f} GB/s  "
              f"read {read / med / 1e6:7.1f} GB/s  {med * 1e3 / n * 1e3:7.2f} us per 1 000 vectors")


def reference(args):
    import importlib.util
    import types
    stub = types.ModuleType("pyserini.index")
    stub.IndexReader = None
    sys.modules.setdefault("pyserini", types.ModuleType("pyserini"))
    sys.modules["pyserini.index"] = stub
    spec = importlib.util.spec_from_file_location("ref_densify_corpus", os.path.join(args.reference, "densify", "densify_corpus.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    n = args.vectors[0]
    indptr, ids, w = vectors(n, args.entries, 2_000_000)
    token2id = {"t%d" % t: t for t in range(2_000_000)}
    data = [{"vector": {"t%d" % t: float(x) for t, x in zip(ids[indptr[b]:indptr[b + 1]], w[indptr[b]:indptr[b + 1]])}} for b in range(n)]
    ns = types.SimpleNamespace(model="bm25")
    t0 = time.perf_counter()
    for d in data:
        ref.densify(d, args.dims, True, token2id, ns)
    dt = time.perf_counter() - t0
    print(f"reference densify, NumPy {np.__version__}, one process: {n} vectors in {dt:.3f} s = {dt / n * 1e3:.4f} s per 1 000 vectors")


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--vectors", type=int, nargs="+", default=None)
    p.add_argument("--entries", type=int, default=60)
    p.add_argument("--dims", type=int, default=768)
    p.add_argument("--reference", default=None)
    a = p.parse_args()
    if a.reference:
        a.vectors = a.vectors or [2000]
        reference(a)
    else:
        a.vectors = a.vectors or [100_000, 1_000_000]
        device(a)
