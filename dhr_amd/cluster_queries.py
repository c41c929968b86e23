"""Query clusters for topic-aware sampling: the `--query_cluster_dir` that the reference's `--tasb_sampling` reads (tevatron/arguments.py:121-137,
tevatron/data.py:205-215) and that nothing in the reference writes.

    python -m dhr_amd.cluster_queries --query_emb_path train.queries.pt --emb_dim 768 --n_clusters 2000 --iters 20 --seed 0 \\
        --output_dir clusters [--columns lo:hi] [--train_file train.jsonl] [--centroids_out c.npy]

The query vectors are clustered on the device (dhr_amd.cluster.kmeans: exactly --iters rounds, the initial centroids drawn by PCG64(--seed),
no atomics: the same flags give the same bytes).  <output_dir>/cluster.json gets one JSON line per non-empty cluster, ordered by cluster:

    {"cluster": j, "size": m, "qidx": [...]}

`qidx`, increasing, is what the training set is indexed with: with --train_file the line position of the record whose `query_id` is the query's
id, without it the position of the query in the pickle.  There is no CPU path: without the HIP library or a GPU the clustering raises."""
from __future__ import annotations

import argparse
import json
import os

import numpy as np


def train_positions(qids, train_file):
    """-> int64 [len(qids)]: the line position in `train_file` of the record of each query (ids compared as strings); a query without a record
    is an error that names it"""
    line_of = {}
    with open(train_file) as f:
        for pos, line in enumerate(f):
            if line.strip():
                line_of.setdefault(str(json.loads(line)["query_id"]), pos)
    out = np.empty(len(qids), np.int64)
    for i, qid in enumerate(qids):
        if str(qid) not in line_of:
            raise KeyError("query {!r} (position {} of the query file) has no record in {}".format(qid, i, train_file))
        out[i] = line_of[str(qid)]
    return out


def cluster_lines(assign, qidx=None):
    """The lines of cluster.json for an assignment [n] -> list of str.  qidx [n]: the training-set position of each query (default: its own)."""
    assign = np.asarray(assign).reshape(-1)
    qidx = np.arange(len(assign), dtype=np.int64) if qidx is None else np.asarray(qidx, np.int64).reshape(-1)
    if len(qidx) != len(assign):
        raise ValueError("{} positions for {} queries".format(len(qidx), len(assign)))
    order = np.argsort(assign, kind="stable")
    bounds = np.flatnonzero(np.diff(assign[order])) + 1
    lines = []
    for members in np.split(order, bounds) if len(order) else []:
        lines.append(json.dumps({"cluster": int(assign[members[0]]), "size": int(len(members)), "qidx": sorted(int(x) for x in qidx[members])}))
    return lines


def write_clusters(output_dir, assign, qidx=None):
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(output_dir, "cluster.json")
    with open(path, "w") as f:
        for line in cluster_lines(assign, qidx):
            f.write(line + "\n")
    return path


def parse_columns(text, emb_dim, width):
    if text is None:
        if width <= emb_dim:
            raise ValueError("the records have no dense tail beyond --emb_dim {} (width {}): name the columns to cluster with --columns lo:hi".format(emb_dim, width))
        return emb_dim, width
    lo, hi = (int(x) for x in text.split(":"))
    if not 0 <= lo < hi <= width:
        raise ValueError("--columns {} outside a record of {} columns".format(text, width))
    return lo, hi


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--query_emb_path", type=str, required=True)
    parser.add_argument("--emb_dim", type=int, default=768, help="DLR dimension: the dense tail starts there")
    parser.add_argument("--n_clusters", type=int, default=2000)
    parser.add_argument("--iters", type=int, default=20, help="rounds of assign + update; all of them run, there is no early stop")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--output_dir", type=str, required=True, help="cluster.json is written there")
    parser.add_argument("--columns", type=str, default=None,
                        help="lo:hi, the columns to cluster; default: the dense tail [emb_dim, width).  The columns are clustered as plain vectors: "
                             "gating by the index array is ignored inside the range")
    parser.add_argument("--train_file", type=str, default=None, help="JSON lines with query_id: qidx becomes the line position of a query's record")
    parser.add_argument("--centroids_out", type=str, default=None, help="also save the final centroids (numpy .npy, float32)")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    from . import _lib, cluster
    from .retrieval import gip_retrieval as G
    _lib.load()                                      # fail before touching the data if the HIP library is missing
    query_embs, _idx, qids = G.load_queries(args.query_emb_path, args.emb_dim, 1)
    columns = parse_columns(args.columns, args.emb_dim, int(query_embs.shape[1]))
    qidx = train_positions(qids, args.train_file) if args.train_file else None
    res = cluster.kmeans(query_embs, args.n_clusters, iters=args.iters, seed=args.seed, columns=columns)
    path = write_clusters(args.output_dir, res.assign, qidx)
    if args.centroids_out:
        np.save(args.centroids_out, res.centroids)
    sizes = res.counts[res.counts > 0]
    print("clustered {} queries into {}: objective {:.6f}, {} empty clusters, sizes {} .. {}".format(
        len(qids), path, float(res.objective[-1]), int((res.counts == 0).sum()), int(sizes.min()), int(sizes.max())))


if __name__ == "__main__":
    main()
