"""`bin_pairs` for the reference's distillation records: what `--kd` reads from every training record (tevatron/data.py:170-198) and nothing
in the reference writes.

    python -m dhr_amd.margin_bins --train_file train.negatives.jsonl --output train.kd.jsonl --n_bins 10 \\
        (--teacher_scores scores.tsv | --query_emb_path train.queries.pt --index_path corpus.index.pt --emb_dim 768)

Every record of --train_file ({"query_id", "positive_pids", "negative_pids", ...}, the output of dhr_amd.mine_negatives) is copied with one
more field, shaped for the consumer's three nested draws:

    bin_pairs = [ per positive: [ per non-empty bin: [ [pos_idx, neg_idx, margin], ... ] ] ]

margin = score(positive) - score(negative); the indices point into the record's own positive_pids / negative_pids.  The bins of a positive
are --n_bins equal-width intervals over the record's margin range (one bin when all margins are equal); empty bins are left out, so no list at
any level is empty.  Scores come from --teacher_scores (`qid pid score` lines, any teacher) or from the index itself: its own gated inner
products (GipIndex.score_rows).  A record without negatives (or without positives) is dropped and counted; a pid without a score is an error
that names it."""
from __future__ import annotations

import argparse
import json

import numpy as np


def read_teacher_scores(path):
    """`qid pid score` lines (blanks or tabs) -> {(qid, pid): score}, ids as strings"""
    scores = {}
    with open(path) as f:
        for n, line in enumerate(f):
            parts = line.split()
            if not parts:
                continue
            if len(parts) != 3:
                raise ValueError("{}:{}: expected `qid pid score`, got {!r}".format(path, n + 1, line.rstrip("\n")))
            scores[(parts[0], parts[1])] = float(parts[2])
    return scores


def bin_pairs(pos_scores, neg_scores, n_bins: int):
    """-> [per positive [per non-empty bin [[pos_idx, neg_idx, margin], ...]]] for one record; both score lists non-empty"""
    if n_bins < 1:
        raise ValueError("n_bins must be >= 1")
    margins = np.asarray(pos_scores, np.float64)[:, None] - np.asarray(neg_scores, np.float64)[None, :]
    lo, hi = float(margins.min()), float(margins.max())
    if hi > lo:
        which = np.minimum(((margins - lo) / (hi - lo) * n_bins).astype(np.int64), n_bins - 1)
    else:
        which = np.zeros(margins.shape, np.int64)
    out = []
    for p in range(margins.shape[0]):
        bins = [[[p, int(j), float(margins[p, j])] for j in np.flatnonzero(which[p] == b)] for b in range(n_bins)]
        out.append([b for b in bins if b])
    return out


def add_bin_pairs(records, score_of, n_bins: int):
    """records: iterable of dicts; score_of(record) -> (scores of positive_pids, scores of negative_pids).  -> (new records, dropped)"""
    out, dropped = [], 0
    for rec in records:
        if not rec.get("positive_pids") or not rec.get("negative_pids"):
            dropped += 1
            continue
        pos, neg = score_of(rec)
        new = dict(rec)
        new["bin_pairs"] = bin_pairs(pos, neg, n_bins)
        out.append(new)
    return out, dropped


def teacher_score_of(scores):
    def score_of(rec):
        qid = str(rec["query_id"])

        def get(pid):
            try:
                return scores[(qid, str(pid))]
            except KeyError:
                raise KeyError("no teacher score for query {!r}, pid {!r}".format(rec["query_id"], pid)) from None
        return [get(p) for p in rec["positive_pids"]], [get(p) for p in rec["negative_pids"]]
    return score_of


def index_scores(records, index, docids, qids, query_embs, query_arg_idxs, batch: int = 1024):
    """The index's own gated inner products of every record's pids -> {position in records: (positive scores, negative scores)}.  Records are
    scored `batch` at a time, each query against its own rows, lists padded to the longest of the batch with the query's first row."""
    wanted = {str(p) for rec in records for p in list(rec["positive_pids"]) + list(rec["negative_pids"])}
    row_of = {}
    for row, docid in enumerate(docids):
        if str(docid) in wanted:
            row_of.setdefault(str(docid), row + index.row_offset)
    q_of = {str(q): i for i, q in enumerate(qids)}
    out = {}
    live = [i for i, rec in enumerate(records) if rec.get("positive_pids") and rec.get("negative_pids")]
    for lo in range(0, len(live), batch):
        part = live[lo:lo + batch]
        lists, qpos = [], []
        for i in part:
            rec = records[i]
            if str(rec["query_id"]) not in q_of:
                raise KeyError("query {!r} is not in the query file".format(rec["query_id"]))
            qpos.append(q_of[str(rec["query_id"])])
            rows = []
            for pid in list(rec["positive_pids"]) + list(rec["negative_pids"]):
                if str(pid) not in row_of:
                    raise KeyError("pid {!r} of query {!r} is not in the index".format(pid, rec["query_id"]))
                rows.append(row_of[str(pid)])
            lists.append(rows)
        m = max(len(r) for r in lists)
        rows = np.asarray([r + [r[0]] * (m - len(r)) for r in lists], np.int64)
        qpos = np.asarray(qpos)
        got = index.score_rows(np.ascontiguousarray(query_embs[qpos]), None if query_arg_idxs is None else np.ascontiguousarray(query_arg_idxs[qpos]), rows)
        for k, i in enumerate(part):
            n_pos = len(records[i]["positive_pids"])
            out[i] = ([float(x) for x in got[k, :n_pos]], [float(x) for x in got[k, n_pos:len(lists[k])]])
    return out


def read_records(path):
    with open(path) as f:
        return [json.loads(line) for line in f if line.strip()]


def write_records(path, records):
    with open(path, "w") as f:
        for rec in records:
            f.write(json.dumps(rec) + "\n")


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--train_file", type=str, required=True, help="JSON lines with query_id, positive_pids, negative_pids")
    parser.add_argument("--output", type=str, required=True, help="the same records with bin_pairs")
    parser.add_argument("--n_bins", type=int, default=10)
    parser.add_argument("--teacher_scores", type=str, default=None, help="`qid pid score` lines")
    parser.add_argument("--query_emb_path", type=str, default=None)
    parser.add_argument("--index_path", type=str, default=None, help="the index pickle, or a device-ready index file")
    parser.add_argument("--emb_dim", type=int, default=768, help="DLR dimension")
    parser.add_argument("--lamda", type=float, default=1, help="weight for [CLS] for concatenation")
    parser.add_argument("--device", type=int, default=0)
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    if (args.teacher_scores is None) == (args.query_emb_path is None or args.index_path is None):
        raise SystemExit("give either --teacher_scores or both --query_emb_path and --index_path")
    records = read_records(args.train_file)
    if args.teacher_scores:
        score_of = teacher_score_of(read_teacher_scores(args.teacher_scores))
    else:
        from . import _lib
        from .retrieval import gip_retrieval as G
        _lib.load()
        query_embs, query_arg_idxs, qids = G.load_queries(args.query_emb_path, args.emb_dim, args.lamda)
        if G.GipIndex.is_device_file(args.index_path):
            index, docids = G.GipIndex.load(args.index_path, device=args.device)
            if docids is None:
                raise ValueError("the device-ready index file carries no docid list")
        else:
            corpus_embs, corpus_arg_idxs, docids, _lo = G.load_corpus_shard(args.index_path)
            if query_arg_idxs is not None and corpus_arg_idxs is None:
                raise ValueError("the query file has an index array but the corpus index has none")
            index = G.GipIndex(corpus_embs, corpus_arg_idxs if query_arg_idxs is not None else None,
                               emb_dim=args.emb_dim if query_arg_idxs is not None else None, device=args.device)
        try:
            table = index_scores(records, index, docids, qids, query_embs, query_arg_idxs)
        finally:
            index.close()
        position = {id(rec): i for i, rec in enumerate(records)}
        score_of = lambda rec: table[position[id(rec)]]          # noqa: E731
    out, dropped = add_bin_pairs(records, score_of, args.n_bins)
    write_records(args.output, out)
    print("wrote {} records with bin_pairs, dropped {} without positives or negatives".format(len(out), dropped))


if __name__ == "__main__":
    main()
