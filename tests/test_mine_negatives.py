"""Hard-negative mining (python -m dhr_amd.mine_negatives) and gip_retrieval --exclude_self.

CPU part: the sampler, the positives reader and the line format, with a numpy stand-in for the index (the mining loop takes any object with
`search(..., exclude=)` and `row_offset`).  GPU part: both command lines end to end on the hybrid corpus of smoke(), from pickles."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from dhr_amd import _lib, mine_negatives as M
from dhr_amd.retrieval import trec
from tests.util import dump_pickle, parse_trec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class NumpyIndex:
    """dense inner product in float64, excluded rows left out, (score desc, row asc), (-inf, -1) padding"""
    row_offset = 0

    def __init__(self, corpus):
        self.c = corpus.astype(np.float64)
        self.batches = []

    def search(self, qv, qi, k, exclude=None):
        self.batches.append(len(qv))
        s = np.asarray(qv, np.float64) @ self.c.T
        out_s, out_r = np.full((len(qv), k), -np.inf, np.float32), np.full((len(qv), k), -1, np.int64)
        for i in range(len(qv)):
            rows = np.setdiff1d(np.arange(s.shape[1]), np.asarray(exclude[i], np.int64))
            order = rows[np.lexsort((rows, -s[i, rows]))][:k]
            out_s[i, :len(order)], out_r[i, :len(order)] = s[i, order], order
        return out_s, out_r


def _mine_text(index, docids, qids, q, lists, pos, **kw):
    import io
    out = io.StringIO()
    M.mine(index, docids, qids, q, None, lists, pos, out=out, **kw)
    return out.getvalue()


def test_sampler_is_seeded_per_query_and_independent_of_the_batch():
    rng = np.random.default_rng(0)
    corpus, q = rng.standard_normal((60, 8)).astype(np.float32), rng.standard_normal((11, 8)).astype(np.float32)
    docids, qids = ["d%d" % i for i in range(60)], ["q%d" % i for i in range(11)]
    positives = {"q%d" % i: ["d%d" % j for j in rng.choice(60, 3, replace=False)] for i in range(0, 11, 2)}
    positives["q2"].append("not-in-the-corpus")
    lists, pos, missing = M.positive_rows(qids, positives, docids)
    assert missing == 1 and [len(x) for x in lists] == [3, 0] * 5 + [3]
    kw = dict(depth=20, n_negatives=5, seed=7)
    texts = {}
    for batch in (1, 3, 4, 100):
        ix = NumpyIndex(corpus)
        texts[batch] = _mine_text(ix, docids, qids, q, lists, pos, batch=batch, **kw)
        assert max(ix.batches) == min(batch, 11)
    assert len(set(texts.values())) == 1                                   # --batch does not change the output
    assert _mine_text(NumpyIndex(corpus), docids, qids, q, lists, pos, batch=4, **kw) == texts[4]           # nor does running it again
    assert _mine_text(NumpyIndex(corpus), docids, qids, q, lists, pos, batch=4, depth=20, n_negatives=5, seed=8) != texts[4]
    recs = [json.loads(ln) for ln in texts[1].splitlines()]
    assert [r["query_id"] for r in recs] == qids
    full = q.astype(np.float64) @ corpus.astype(np.float64).T
    for i, r in enumerate(recs):
        assert list(r) == ["query_id", "positive_pids", "negative_pids"]
        assert r["positive_pids"] == positives.get(qids[i], [])
        assert len(r["negative_pids"]) == 5 == len(set(r["negative_pids"])) and not set(r["negative_pids"]) & set(r["positive_pids"])
        allowed = [j for j in np.lexsort((np.arange(60), -full[i])) if docids[j] not in r["positive_pids"]][:20]
        assert set(r["negative_pids"]) <= {docids[j] for j in allowed}
    # the draw of a query follows from (seed, position, its list) alone
    cand = ["d%d" % j for j in range(40)]
    assert M.sample_negatives(cand, 7, 3, 5) == M.sample_negatives(cand, 7, 3, 5) != M.sample_negatives(cand, 7, 4, 5)
    want = np.random.Generator(np.random.PCG64([7, 3])).choice(40, size=5, replace=False)
    assert M.sample_negatives(cand, 7, 3, 5) == [cand[j] for j in want]


def test_fewer_survivors_than_n_negatives_give_a_shorter_list():
    corpus = np.eye(6, dtype=np.float32)
    docids, qids = list("abcdef"), ["q"]
    lists, pos, missing = M.positive_rows(qids, {"q": ["a", "c"]}, docids)
    text = _mine_text(NumpyIndex(corpus), docids, qids, corpus[:1], lists, pos, depth=50, n_negatives=30, seed=0, batch=8)
    rec = json.loads(text)
    assert missing == 0 and sorted(rec["negative_pids"]) == ["b", "d", "e", "f"] and rec["positive_pids"] == ["a", "c"]
    assert M.sample_negatives([], 0, 0, 30) == []


def test_json_line_format_and_integer_ids():
    line = M.json_line(np.int64(7), [np.int32(3)], ["x", 5])
    assert line == '{"query_id": 7, "positive_pids": [3], "negative_pids": ["x", 5]}'
    # integer ids in the pickles match the strings of a qrels file
    lists, pos, missing = M.positive_rows([11], {"11": ["5", "9"]}, [4, 5, 6], row_base=100)
    assert lists[0].tolist() == [101] and pos == [["5", "9"]] and missing == 1


def test_positives_reader_takes_qrels_and_pair_files(tmp_path):
    (tmp_path / "tab.tsv").write_text("q1\t0\td3\t1\nq1\t0\td4\t0\nq2\t0\td9\t2\n")
    (tmp_path / "trec.txt").write_text("q1 0 d3 1\nq2 0 d9 1\n\n")
    (tmp_path / "pairs.txt").write_text("q1 d3\nq2\td9\nq1 d7\n")
    assert M.read_positives(str(tmp_path / "tab.tsv")) == {"q1": ["d3"], "q2": ["d9"]}
    assert M.read_positives(str(tmp_path / "trec.txt")) == {"q1": ["d3"], "q2": ["d9"]}
    assert M.read_positives(str(tmp_path / "pairs.txt")) == {"q1": ["d3", "d7"], "q2": ["d9"]}
    (tmp_path / "bad.txt").write_text("q1 d3 1\n")
    with pytest.raises(ValueError):
        trec.read_qrels_any(str(tmp_path / "bad.txt"))


def test_make_exclusions_round_trips_lists_and_csr():
    lists = [[5, 1, 1], [], np.array([1 << 40, -1], np.int64), range(3)]
    ptr, rows, kind, keep = _lib.make_exclusions(lists)
    assert ptr.dtype == np.int64 and ptr.tolist() == [0, 3, 3, 5, 8] and kind == _lib.MEM_HOST and keep is not None
    assert rows.dtype == np.int64 and rows.tolist() == [5, 1, 1, 1 << 40, -1, 0, 1, 2]
    assert [rows[ptr[q]:ptr[q + 1]].tolist() for q in range(4)] == [list(map(int, x)) for x in lists]
    ptr2, rows2, kind2, _ = _lib.make_exclusions((ptr.astype(np.int32), rows))
    assert ptr2.dtype == np.int64 and ptr2.tolist() == ptr.tolist() and rows2 is rows and kind2 == _lib.MEM_HOST
    e_ptr, e_rows, _, _ = _lib.make_exclusions([])
    assert e_ptr.tolist() == [0] and e_rows.shape == (0,)
    with pytest.raises(_lib.DhrError):
        _lib.make_exclusions((np.array([0, 2], np.int64), np.zeros(3, np.int64)))
    with pytest.raises(_lib.DhrError):
        _lib.make_exclusions((ptr, rows, rows))


# ------------------------------------------------------------------------------------------ GPU: the command lines
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the hybrid corpus of smoke() as pickles; the query set is 12 corpus rows under their own docids plus 4 ordinary queries"""
    from dhr_amd import synth
    d = tmp_path_factory.mktemp("mine")
    cv, ci, qv, qi = synth.make_pair(5, 3000, 8, 768, 128)
    docids = ["d%d" % i for i in range(3000)]
    own = np.random.default_rng(2).choice(3000, 12, replace=False)
    q_val = np.concatenate([cv[own], qv[:4]])
    q_idx = np.concatenate([ci[own], qi[:4]])
    qids = [docids[r] for r in own] + ["q%d" % i for i in range(4)]
    dump_pickle(str(d / "c.pt"), cv, ci, docids)
    dump_pickle(str(d / "q.pt"), q_val, q_idx, qids)
    return dict(dir=d, cv=cv, ci=ci, q_val=q_val, q_idx=q_idx, qids=qids, docids=docids, own=own)


@pytest.mark.gpu
def test_mine_negatives_command_line(files):
    from oracle import gip_oracle as O
    d, qids, docids = files["dir"], files["qids"], files["docids"]
    rng = np.random.default_rng(3)
    positives = {qid: ["d%d" % j for j in rng.choice(3000, 4, replace=False)] for qid in qids[:14]}
    for i, r in enumerate(files["own"]):
        positives[qids[i]] = list(dict.fromkeys(positives[qids[i]] + [docids[r]]))     # the query's own passage is a positive, as in a corpus mined against itself
    positives[qids[0]].append("d999999")
    with open(d / "pos.tsv", "w") as f:
        for qid, pids in positives.items():
            for pid in pids:
                f.write("%s\t0\t%s\t1\n" % (qid, pid))
    depth, n_neg = 50, 10
    argv = ["--query_emb_path", str(d / "q.pt"), "--index_path", str(d / "c.pt"), "--emb_dim", "768", "--positives", str(d / "pos.tsv"), "--depth", str(depth),
            "--n_negatives", str(n_neg), "--seed", "3"]
    run = subprocess.run([sys.executable, "-m", "dhr_amd.mine_negatives"] + argv + ["--batch", "5", "--output", str(d / "a.jsonl"), "--run_file", str(d / "a.trec")],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "1 positive pids are not in the corpus" in run.stdout
    M.main(argv + ["--batch", "4096", "--output", str(d / "b.jsonl"), "--run_file", str(d / "b.trec")])       # (the same entry point, in this process)
    outs = [(open(d / (name + ".jsonl")).read(), open(d / (name + ".trec")).read()) for name in "ab"]
    assert outs[0] == outs[1]                                 # --batch changes neither file
    recs = [json.loads(ln) for ln in outs[0][0].splitlines()]
    runs = parse_trec(outs[0][1])
    assert [r["query_id"] for r in recs] == qids
    c32, q32 = files["cv"].astype(np.float32), files["q_val"].astype(np.float32)
    for i, rec in enumerate(recs):
        pos = positives.get(qids[i], [])
        assert rec["positive_pids"] == pos and len(rec["negative_pids"]) == n_neg == len(set(rec["negative_pids"]))
        ex = O.gip_scores_f64(q32[i], files["q_idx"][i], c32, files["ci"])
        remain = np.array([j for j in range(3000) if docids[j] not in pos])
        # the run file holds the filtered top-`depth`, checked as smoke() checks a search; the negatives are drawn from it
        listed = [(int(did[1:]), rank, score) for did, rank, score in runs[qids[i]]]
        assert [r for _, r, _ in listed] == list(range(1, depth + 1))
        O.check_topk(np.searchsorted(remain, [j for j, _, _ in listed]), [s for _, _, s in listed], ex[remain], depth)
        assert set(rec["negative_pids"]) <= {"d%d" % j for j, _, _ in listed} and not set(rec["negative_pids"]) & set(pos)


MODES = {"brute": ["--brute_force"], "theta_rerank": ["--theta", "0.1", "--rerank", "--agip_topk", "60"], "ip_rerank": ["--IP", "--rerank", "--agip_topk", "60"],
         "pqip": ["--PQIP", "--agip_topk", "200"], "pqip_rerank": ["--PQIP", "--rerank", "--agip_topk", "200"]}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_exclude_self_writes_k_lines_with_contiguous_ranks(files, mode, monkeypatch):
    from dhr_amd.retrieval import gip_retrieval as G
    d, qids, k = files["dir"], files["qids"], 10
    monkeypatch.chdir(d)
    base = ["--query_emb_path", "q.pt", "--index_path", "c.pt", "--emb_dim", "768", "--topk", str(k)] + MODES[mode]
    if mode.startswith("pqip"):
        if not os.path.exists("pq_index"):
            from dhr_amd.retrieval import quantize_index as QI
            QI.main(["--index_path", "c.pt", "--output_index_path", "pq_index"])
        base += ["--faiss_pq_index_path", "pq_index"]
    G.main(base + ["--output", mode + ".plain.trec"])
    G.main(base + ["--exclude_self", "--output", mode + ".self.trec"])
    plain, filtered = parse_trec(open(mode + ".plain.trec").read()), parse_trec(open(mode + ".self.trec").read())
    assert list(filtered) == qids
    for i, qid in enumerate(qids):
        docs, ranks = [x[0] for x in filtered[qid]], [x[1] for x in filtered[qid]]
        assert ranks == list(range(1, k + 1)) and qid not in docs and len(set(docs)) == k, (mode, qid, ranks)
        plain_docs, plain_ranks = [x[0] for x in plain[qid]], [x[1] for x in plain[qid]]
        if i >= 12:                                            # a query that is no corpus document: the flag changes nothing
            assert filtered[qid] == plain[qid]
            continue
        # today's run drops the docid == query_id line while writing and leaves its rank unused; the others keep their order either way
        assert qid not in plain_docs and docs[: len(plain_docs)] == plain_docs
        assert len(plain_docs) in (k - 1, k) and len(set(range(1, k + 1)) - set(plain_ranks)) == k - len(plain_docs)
        if mode == "brute":                                    # a passage is among its own ten best under the exact score
            assert len(plain_docs) == k - 1


@pytest.mark.gpu
def test_without_the_flag_the_run_file_is_what_the_plain_search_and_the_reference_writer_give(files, monkeypatch):
    """(the byte comparison against the parent commit's own run is made once, by hand, when the change is reviewed: profiles/search_excluding.txt)"""
    import io
    from dhr_amd.retrieval import gip_retrieval as G
    d, qids, docids = files["dir"], files["qids"], files["docids"]
    monkeypatch.chdir(d)
    G.main(["--query_emb_path", "q.pt", "--index_path", "c.pt", "--emb_dim", "768", "--topk", "10", "--brute_force", "--output", "noflag.trec"])
    ix = G.GipIndex(files["cv"], files["ci"])
    scores, rows = ix.search(files["q_val"].astype(np.float32), files["q_idx"], 10)
    ix.close()
    want = io.StringIO()
    G.write_trec(want, *G._to_dicts(qids, rows, scores), docids, "h2oloo")
    assert open("noflag.trec").read() == want.getvalue()
