"""The two files that the reference's TAS-B / KD training set reads and nothing in the reference writes: query clusters
(python -m dhr_amd.cluster_queries -> cluster.json, tevatron/data.py:205-215) and bin_pairs (python -m dhr_amd.margin_bins, data.py:170-198).

The consumer's walks are restated here in a few lines (`draw_pairs`, the three nested random.choices of data.py:176-196) and run over every
record with many seeds: every draw must land on a valid positive and a valid negative and return that pair's margin.

CPU part (-m "not gpu"): the file writers from a given assignment, margin_bins from a teacher-score file.  GPU part: cluster_queries end to end."""
import json
import os
import pickle
import random

import numpy as np
import pytest

from dhr_amd import cluster_queries as CQ
from dhr_amd import margin_bins as MB


# ------------------------------------------------------------------------------------------ cluster_queries: file writing
def _read_clusters(path):
    with open(path) as f:
        return [json.loads(line) for line in f]


def test_cluster_file_from_a_given_assignment(tmp_path):
    rng = np.random.Generator(np.random.PCG64(1))
    n, K = 200, 12
    assign = rng.integers(0, K, n).astype(np.int32)
    assign[np.isin(assign, (0, 5, 11))] = 4                      # empty clusters: the first, one inside, the last
    path = CQ.write_clusters(str(tmp_path / "clusters"), assign)
    assert path == str(tmp_path / "clusters" / "cluster.json")
    lines = _read_clusters(path)
    assert [c["cluster"] for c in lines] == sorted(set(assign.tolist())) and not {0, 5, 11} & {c["cluster"] for c in lines}
    seen = []
    for c in lines:
        assert set(c) == {"cluster", "size", "qidx"}
        assert c["size"] == len(c["qidx"]) > 0 and c["qidx"] == sorted(c["qidx"])
        assert all(assign[i] == c["cluster"] for i in c["qidx"])
        seen += c["qidx"]
    assert sorted(seen) == list(range(n))                         # every position in exactly one line
    # the consumer's draw (data.py:208-213) lands on a query of the drawn cluster
    random.seed(3)
    for _ in range(50):
        cluster = random.choices(random.choices(lines, k=24), k=1)[0]
        item = random.choices(cluster["qidx"])[0]
        assert assign[item] == cluster["cluster"]


def test_cluster_file_with_a_train_file(tmp_path):
    rng = np.random.Generator(np.random.PCG64(2))
    n = 60
    qids = ["q%d" % i for i in range(n)]
    order = rng.permutation(n + 5)                                # the training file holds the queries in another order, and five more
    train = tmp_path / "train.jsonl"
    with open(train, "w") as f:
        for pos in range(n + 5):
            k = int(np.flatnonzero(order == pos)[0])
            f.write(json.dumps({"query_id": qids[k] if k < n else "extra%d" % k, "positive_pids": [1], "negative_pids": [2]}) + "\n")
    qidx = CQ.train_positions(qids, str(train))
    assert np.array_equal(qidx, order[:n])
    assign = rng.integers(0, 7, n)
    lines = _read_clusters(CQ.write_clusters(str(tmp_path / "c"), assign, qidx))
    seen = [p for c in lines for p in c["qidx"]]
    assert sorted(seen) == sorted(order[:n].tolist()) and len(set(seen)) == n
    records = [json.loads(line) for line in open(train)]
    for c in lines:
        assert c["qidx"] == sorted(c["qidx"])
        for p in c["qidx"]:
            assert assign[qids.index(records[p]["query_id"])] == c["cluster"]
    # integer ids in the pickle match string ids in the file; an absent query is an error that names it
    with open(train, "w") as f:
        f.write(json.dumps({"query_id": "7"}) + "\n" + json.dumps({"query_id": 8}) + "\n")
    assert CQ.train_positions([8, 7], str(train)).tolist() == [1, 0]
    with pytest.raises(KeyError, match="'q-absent'"):
        CQ.train_positions([7, "q-absent"], str(train))


def test_cluster_queries_flags_and_columns():
    args = CQ.build_parser().parse_args(["--query_emb_path", "q.pt", "--output_dir", "out"])
    assert (args.emb_dim, args.n_clusters, args.iters, args.seed, args.columns, args.train_file, args.centroids_out) == (768, 2000, 20, 0, None, None, None)
    assert "gating" in CQ.build_parser().format_help() and "ignored" in CQ.build_parser().format_help()
    assert CQ.parse_columns(None, 768, 1536) == (768, 1536)
    assert CQ.parse_columns("10:20", 768, 768) == (10, 20)
    with pytest.raises(ValueError, match="--columns"):
        CQ.parse_columns(None, 768, 768)
    with pytest.raises(ValueError, match="outside"):
        CQ.parse_columns("10:800", 768, 768)


# ------------------------------------------------------------------------------------------ margin_bins
def draw_pairs(group, n_passages, rng):
    """data.py:176-196 -> (positive pid, [negative pids], [teacher scores])"""
    bins_pairs = rng.choices(group["bin_pairs"], k=1)[0]
    pairs = []
    for _ in range(n_passages - 1):
        bin_pairs = rng.choices(bins_pairs, k=1)[0]
        pairs.append(rng.choices(bin_pairs, k=1)[0])
    pos = group["positive_pids"][int(pairs[0][0])]
    return pos, [group["negative_pids"][int(p[1])] for p in pairs], [-p[2] for p in pairs], pairs


def _records(tmp_path, seed=4, n=25):
    rng = np.random.Generator(np.random.PCG64(seed))
    records, scores = [], {}
    for q in range(n):
        n_pos, n_neg = int(rng.integers(1, 4)), int(rng.integers(1, 40))
        pids = rng.permutation(10_000)[:n_pos + n_neg].tolist()
        rec = {"query_id": "q%d" % q if q % 2 else q, "query": [1, 2, 3], "positive_pids": pids[:n_pos], "negative_pids": [str(p) for p in pids[n_pos:]]}
        records.append(rec)
        for p in pids:
            scores[(str(rec["query_id"]), str(p))] = float(np.round(rng.normal(0, 3), 3))
    train, tsv = tmp_path / "train.jsonl", tmp_path / "scores.tsv"
    MB.write_records(str(train), records)
    with open(tsv, "w") as f:
        for (q, p), s in scores.items():
            f.write("%s\t%s\t%r\n" % (q, p, s))
    return records, scores, str(train), str(tsv)


def test_margin_bins_from_teacher_scores(tmp_path, capsys):
    records, scores, train, tsv = _records(tmp_path)
    out = str(tmp_path / "train.kd.jsonl")
    MB.main(["--train_file", train, "--output", out, "--n_bins", "10", "--teacher_scores", tsv])
    text = capsys.readouterr().out
    assert "wrote 25 records" in text and "dropped 0" in text
    got = MB.read_records(out)
    assert len(got) == len(records)
    for rec, new in zip(records, got):
        assert {k: v for k, v in new.items() if k != "bin_pairs"} == rec                # every field is copied
        bp = new["bin_pairs"]
        n_pos, n_neg = len(rec["positive_pids"]), len(rec["negative_pids"])
        assert len(bp) == n_pos
        s = lambda pid: scores[(str(rec["query_id"]), str(pid))]                       # noqa: E731
        margins = np.asarray([[s(p) - s(q) for q in rec["negative_pids"]] for p in rec["positive_pids"]])
        lo, hi = margins.min(), margins.max()
        for p, bins in enumerate(bp):
            assert 1 <= len(bins) <= 10 and all(len(b) > 0 for b in bins)             # no empty list at any level
            pairs = [tuple(x) for b in bins for x in b]
            assert sorted(x[1] for x in pairs) == list(range(n_neg)) and all(x[0] == p for x in pairs)      # every negative in exactly one bin
            for b in bins:
                for pi, ni, m in b:
                    assert m == pytest.approx(margins[pi, ni], abs=1e-12)
                if hi > lo:                                                            # equal-width intervals over the record's margin range
                    ks = {min(int((m - lo) / (hi - lo) * 10), 9) for _, _, m in b}
                    assert len(ks) == 1
        # the consumer's walk, many seeds
        for seed in range(40):
            rng = random.Random(1000 * seed + n_neg)
            pos, negs, teacher, pairs = draw_pairs(new, 8, rng)
            assert pos in rec["positive_pids"] and len(negs) == 7 and all(x in rec["negative_pids"] for x in negs)
            for x, neg, t in zip(pairs, negs, teacher):
                assert rec["positive_pids"][int(x[0])] == pos
                assert t == pytest.approx(-(s(pos) - s(neg)), abs=1e-12)


def test_margin_bins_edge_cases(tmp_path, capsys):
    # all margins equal: one bin
    assert MB.bin_pairs([2.0, 2.0], [1.0, 1.0, 1.0], 10) == [[[[0, 0, 1.0], [0, 1, 1.0], [0, 2, 1.0]]], [[[1, 0, 1.0], [1, 1, 1.0], [1, 2, 1.0]]]]
    assert MB.bin_pairs([5.0], [1.0], 4) == [[[[0, 0, 4.0]]]]
    # the largest margin falls into the last bin, the smallest into the first
    bp = MB.bin_pairs([1.0], [0.0, 0.5, 1.0], 2)
    assert bp == [[[[0, 2, 0.0]], [[0, 0, 1.0], [0, 1, 0.5]]]]
    # a record without negatives is dropped and counted; a pid without a score is an error that names it
    train, tsv, out = tmp_path / "t.jsonl", tmp_path / "s.tsv", tmp_path / "o.jsonl"
    MB.write_records(str(train), [{"query_id": 1, "positive_pids": [10], "negative_pids": []},
                                  {"query_id": 2, "positive_pids": [10], "negative_pids": [11, 12]}])
    open(tsv, "w").write("2 10 1.5\n2 11 0.5\n2 12 -1\n")
    MB.main(["--train_file", str(train), "--output", str(out), "--teacher_scores", str(tsv)])
    assert "wrote 1 records" in capsys.readouterr().out
    got = MB.read_records(str(out))
    assert len(got) == 1 and got[0]["query_id"] == 2 and sum(len(b) for b in got[0]["bin_pairs"][0]) == 2
    open(tsv, "w").write("2 10 1.5\n2 11 0.5\n")
    with pytest.raises(KeyError, match="pid 12"):
        MB.main(["--train_file", str(train), "--output", str(out), "--teacher_scores", str(tsv)])
    with pytest.raises(SystemExit):
        MB.main(["--train_file", str(train), "--output", str(out)])
    open(tsv, "w").write("2 10\n")
    with pytest.raises(ValueError, match="qid pid score"):
        MB.read_teacher_scores(str(tsv))


# ------------------------------------------------------------------------------------------ GPU part
@pytest.mark.gpu
def test_cluster_queries_end_to_end(tmp_path, capsys):
    from dhr_amd import synth
    n = 600
    _cv, _ci, qv, qi = synth.make_pair(11, 64, n, d_dlr=64, d_cls=48)
    qids = ["q%d" % i for i in range(n)]
    pt = tmp_path / "train.queries.pt"
    with open(pt, "wb") as f:
        pickle.dump([qv, qi, qids], f, protocol=4)
    files = []
    for run in ("a", "b"):
        out = tmp_path / run
        CQ.main(["--query_emb_path", str(pt), "--emb_dim", "64", "--n_clusters", "8", "--iters", "5", "--seed", "0", "--output_dir", str(out),
                 "--centroids_out", str(tmp_path / (run + ".npy"))])
        text = capsys.readouterr().out
        assert "clustered 600 queries" in text and "empty clusters" in text
        files.append(open(out / "cluster.json", "rb").read())
    assert files[0] == files[1]                                   # a second run gives a byte-identical file
    lines = [json.loads(x) for x in files[0].decode().splitlines()]
    assert sorted(p for c in lines for p in c["qidx"]) == list(range(n))
    assert [c["cluster"] for c in lines] == sorted(c["cluster"] for c in lines) and all(c["size"] == len(c["qidx"]) for c in lines)
    cen = np.load(tmp_path / "a.npy")
    assert cen.shape == (8, 48) and cen.dtype == np.float32 and np.array_equal(cen, np.load(tmp_path / "b.npy"))
    # the file agrees with the nearest of the saved centroids on the dense tail, up to ties
    x = np.asarray(qv)[:, 64:].astype(np.float64)
    t = x @ cen.astype(np.float64).T - 0.5 * (cen.astype(np.float64) ** 2).sum(1)[None, :]
    where = np.empty(n, np.int64)
    for c in lines:
        where[c["qidx"]] = c["cluster"]
    assert (t.max(1) - t[np.arange(n), where] <= 1e-5).all()
    # --train_file: positions of the records, in another order
    order = np.random.Generator(np.random.PCG64(0)).permutation(n)
    train = tmp_path / "train.jsonl"
    with open(train, "w") as f:
        for pos in range(n):
            f.write(json.dumps({"query_id": qids[int(np.flatnonzero(order == pos)[0])]}) + "\n")
    CQ.main(["--query_emb_path", str(pt), "--emb_dim", "64", "--n_clusters", "8", "--iters", "5", "--output_dir", str(tmp_path / "c"), "--train_file", str(train)])
    mapped = [json.loads(x) for x in open(tmp_path / "c" / "cluster.json")]
    assert [sorted(int(order[p]) for p in c["qidx"]) for c in lines] == [c["qidx"] for c in mapped]


@pytest.mark.gpu
def test_margin_bins_from_the_index(tmp_path, capsys):
    """the score source is the index itself: margins are differences of its gated inner products (GipIndex.score_rows, no new kernel)"""
    from dhr_amd import synth
    from oracle import gip_oracle as O
    n, nq = 500, 6
    cv, ci, qv, qi = synth.make_pair(12, n, nq, d_dlr=64, d_cls=32)
    docids, qids = ["d%d" % i for i in range(n)], list(range(100, 100 + nq))
    with open(tmp_path / "corpus.pt", "wb") as f:
        pickle.dump([cv, ci, docids], f, protocol=4)
    with open(tmp_path / "q.pt", "wb") as f:
        pickle.dump([qv, qi, qids], f, protocol=4)
    rng = np.random.Generator(np.random.PCG64(3))
    records = []
    for k, q in enumerate(qids):
        rows = rng.permutation(n)[:2 + 3 * k + 1]
        records.append({"query_id": q, "positive_pids": [docids[r] for r in rows[:1 + k % 2]], "negative_pids": [docids[r] for r in rows[1 + k % 2:]]})
    records.append({"query_id": qids[0], "positive_pids": [docids[0]], "negative_pids": []})
    MB.write_records(str(tmp_path / "train.jsonl"), records)
    MB.main(["--train_file", str(tmp_path / "train.jsonl"), "--output", str(tmp_path / "kd.jsonl"), "--n_bins", "4", "--query_emb_path", str(tmp_path / "q.pt"),
             "--index_path", str(tmp_path / "corpus.pt"), "--emb_dim", "64"])
    text = capsys.readouterr().out
    assert "wrote 6 records" in text and "dropped 1" in text
    got = MB.read_records(str(tmp_path / "kd.jsonl"))
    assert len(got) == nq
    row_of = {d: i for i, d in enumerate(docids)}
    for k, new in enumerate(got):
        ex = O.gip_scores_f64(qv[k].astype(np.float32), qi[k], cv.astype(np.float32), ci)
        seen = set()
        for bins in new["bin_pairs"]:
            assert bins and all(bins)
            for b in bins:
                for pi, ni, m in b:
                    want = ex[row_of[new["positive_pids"][pi]]] - ex[row_of[new["negative_pids"][ni]]]
                    assert abs(m - want) <= 1e-3 * (1 + abs(want))
                    seen.add((pi, ni))
        assert len(seen) == len(new["positive_pids"]) * len(new["negative_pids"])
    MB.write_records(str(tmp_path / "bad.jsonl"), [{"query_id": qids[1], "positive_pids": ["d1"], "negative_pids": ["nope"]}])
    with pytest.raises(KeyError, match="nope"):
        MB.main(["--train_file", str(tmp_path / "bad.jsonl"), "--output", str(tmp_path / "o.jsonl"), "--query_emb_path", str(tmp_path / "q.pt"),
                 "--index_path", str(tmp_path / "corpus.pt"), "--emb_dim", "64"])
