"""Hard-negative mining on the device: the `negative_pids` of the reference's training records (docs/dhr/msmarco-passage-train-eval.md:13).

    python -m dhr_amd.mine_negatives --query_emb_path train.queries.pt --index_path corpus.index.pt --emb_dim 768 \\
        --positives qrels.train.tsv --depth 200 --n_negatives 30 --seed 0 --output train.negatives.jsonl [--run_file train.trec]

Each query's positives (a qrels file, or `qid pid` lines) become its exclusion list; the exact search runs `--depth` deep with those rows
excluded on the device (dhr_search_excluding: no list leaves the GPU deeper than it is written), and `--n_negatives` of the result are
drawn without replacement by numpy.random.Generator(PCG64([seed, position of the query in the query file])) -- the draw of a query depends
on nothing but the seed, its position and its list, so --batch changes nothing.  One JSON line per query, in query order:

    {"query_id": ..., "positive_pids": [...], "negative_pids": [...]}

the fields a training record carries besides the query tokens.  Ids are written as the query and index files hold them.  A query with
fewer than --n_negatives results keeps what there is; positives that are not in the corpus are counted and reported once at the end.
--run_file also writes the filtered lists as a TREC run (the library's writer).  There is no CPU path: without the HIP library or a GPU
the search raises."""
from __future__ import annotations

import argparse
import json

import numpy as np

from .retrieval import trec


def read_positives(path):
    """-> {qid: [pid, ...]} the pids with rel > 0 of a qrels file (either layout of trec.read_qrels_any) or of `qid pid` lines, in file order"""
    return {qid: [pid for pid, rel in judged.items() if rel > 0] for qid, judged in trec.read_qrels_any(path).items()}


def positive_rows(qids, positives, docids, row_base=0):
    """-> (per-query int64 arrays of global rows, per-query lists of positive pids, number of positive pids that are not in the corpus).
    Ids are compared as strings, so a qrels file matches a pickle that holds integer ids."""
    wanted = {pid for qid in qids for pid in positives.get(str(qid), ())}
    row_of = {}
    for row, docid in enumerate(docids):
        if str(docid) in wanted:
            row_of.setdefault(str(docid), []).append(row + row_base)
    lists, pids, missing = [], [], 0
    for qid in qids:
        pos = list(positives.get(str(qid), ()))
        missing += sum(1 for pid in pos if pid not in row_of)
        lists.append(np.asarray([r for pid in pos for r in row_of.get(pid, ())], np.int64))
        pids.append(pos)
    return lists, pids, missing


def sample_negatives(candidates, seed: int, position: int, n: int):
    """n of the candidates (fewer where there are fewer) without replacement, in the order drawn; the generator is seeded from (seed, position) alone"""
    rng = np.random.Generator(np.random.PCG64([int(seed), int(position)]))
    take = min(int(n), len(candidates))
    return [candidates[i] for i in rng.choice(len(candidates), size=take, replace=False)] if take else []


def _plain(x):
    return x.item() if isinstance(x, np.generic) else x


def json_line(qid, positive_pids, negative_pids) -> str:
    return json.dumps({"query_id": _plain(qid), "positive_pids": [_plain(p) for p in positive_pids], "negative_pids": [_plain(p) for p in negative_pids]})


def mine(index, docids, qids, query_embs, query_arg_idxs, lists, pos_pids, *, depth, n_negatives, seed, batch, out, run_file=None, run_name="dhr"):
    """The loop of main() over an open GipIndex: search `depth` deep with the exclusion lists, sample, write one line per query to `out`."""
    from .retrieval import gip_retrieval as G
    batch = max(1, min(int(batch), G.QUERY_CHUNK))
    for lo in range(0, len(qids), batch):
        hi = min(len(qids), lo + batch)
        scores, rows = index.search(query_embs[lo:hi], None if query_arg_idxs is None else query_arg_idxs[lo:hi], depth, exclude=lists[lo:hi])
        for i in range(hi - lo):
            cand = [docids[r] for r in (rows[i][rows[i] >= 0] - index.row_offset)]
            out.write(json_line(qids[lo + i], pos_pids[lo + i], sample_negatives(cand, seed, lo + i, n_negatives)) + "\n")
        if run_file and G.write_trec_native(run_file, qids[lo:hi], rows, scores, index.row_offset, docids, run_name, append=lo > 0) is None:
            with open(run_file, "a" if lo > 0 else "w") as f:
                G.write_trec(f, *G._to_dicts(qids[lo:hi], rows, scores, index.row_offset), docids, run_name)


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--query_emb_path", type=str, required=True)
    parser.add_argument("--index_path", type=str, required=True, help="the index pickle, or a device-ready index file")
    parser.add_argument("--emb_dim", type=int, default=768, help="DLR dimension")
    parser.add_argument("--lamda", type=float, default=1, help="weight for [CLS] for concatenation")
    parser.add_argument("--positives", type=str, required=True, help="qrels (4 columns) or `qid pid` lines")
    parser.add_argument("--depth", type=int, default=200, help="negatives are drawn from the `depth` best rows that are not positives")
    parser.add_argument("--n_negatives", type=int, default=30)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--batch", type=int, default=4096, help="queries per search call (does not change the output)")
    parser.add_argument("--output", type=str, required=True, help="JSON lines: query_id, positive_pids, negative_pids")
    parser.add_argument("--run_file", type=str, default=None, help="also write the filtered top-`depth` lists as a TREC run")
    parser.add_argument("--run_name", type=str, default="dhr")
    parser.add_argument("--device", type=int, default=0)
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    from . import _lib
    from .retrieval import gip_retrieval as G
    _lib.load()                                      # fail before touching the data if the HIP library is missing
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
    lists, pos_pids, missing = positive_rows(qids, read_positives(args.positives), docids, index.row_offset)
    try:
        with open(args.output, "w") as out:
            mine(index, docids, qids, query_embs, query_arg_idxs, lists, pos_pids, depth=args.depth, n_negatives=args.n_negatives, seed=args.seed,
                 batch=args.batch, out=out, run_file=args.run_file, run_name=args.run_name)
    finally:
        index.close()
    print('mined {} queries, {} positive pids are not in the corpus'.format(len(qids), missing))


if __name__ == "__main__":
    main()
