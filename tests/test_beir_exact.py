"""dhr_amd.beir_exact.ExactSearch against a numpy restatement of BEIR's exact dense search: a fake model whose embeddings are a function of the
text, and a stand-in for StreamSearch that keeps every score in numpy.  Covered: the corpus taken longest text first and in chunks, the chunk
boundaries and their row numbers, the document whose id is the query's dropped, fewer documents than top_k, the score function.  CPU only: the
device path of StreamSearch is tests/test_stream_search.py."""
import zlib

import numpy as np
import pytest

from dhr_amd import beir_exact

D = 12


def _embed(text):
    """a small non-negative integer vector per text: every inner product is exact in fp32, and ties happen"""
    rng = np.random.Generator(np.random.PCG64(zlib.crc32(text.encode())))
    return rng.integers(0, 4, D).astype(np.float32)


class FakeModel:
    sep = " "

    def __init__(self):
        self.corpus_calls, self.query_calls = [], []

    def encode_queries(self, queries, batch_size, **kw):
        self.query_calls.append((list(queries), batch_size))
        return np.stack([_embed(t) for t in queries])

    def encode_corpus(self, corpus, batch_size, **kw):
        texts = [(doc["title"] + self.sep + doc["text"]).strip() for doc in corpus]
        self.corpus_calls.append((texts, batch_size))
        return np.stack([_embed(t) for t in texts])


class NumpySearch:
    """what StreamSearch computes, in float64 on the host"""
    made = []

    def __init__(self, q_a, q_b=None, k=1000, block_rows=0):
        assert q_b is None
        self.q, self.k, self.scores, self.rows, self.adds = np.asarray(q_a, np.float64), k, [], [], []
        NumpySearch.made.append(self)

    def add(self, p_a, p_b=None, row_base=None):
        assert p_b is None and row_base is not None
        self.adds.append((int(row_base), len(p_a)))
        self.scores.append(self.q @ np.asarray(p_a, np.float64).T)
        self.rows.append(np.arange(row_base, row_base + len(p_a), dtype=np.int64))
        return self

    def result(self):
        s, r = np.concatenate(self.scores, 1), np.concatenate(self.rows)
        out_s, out_r = np.full((len(self.q), self.k), -np.inf, np.float32), np.full((len(self.q), self.k), -1, np.int64)
        for i in range(len(self.q)):
            o = np.lexsort((r, -s[i]))[:self.k]
            out_s[i, :len(o)], out_r[i, :len(o)] = s[i, o], r[o]
        return out_s, out_r

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.closed = True


def _data(n_docs, n_queries=6):
    rng = np.random.Generator(np.random.PCG64(11))
    words = ["alpha", "beta", "gamma", "delta", "epsilon", "zeta", "eta", "theta"]
    text = lambda n: " ".join(rng.choice(words, n))            # noqa: E731
    corpus = {"d%d" % i: {"title": text(rng.integers(0, 3)), "text": text(rng.integers(1, 30))} for i in range(n_docs)}
    queries = {"q%d" % i: text(rng.integers(2, 6)) for i in range(n_queries)}
    # two queries whose ids are corpus ids (the argument-retrieval corpora of BEIR): their own document must not come back
    for docid in list(corpus)[:2]:
        queries[docid] = corpus[docid]["text"]
    return corpus, queries


def _restatement(corpus, queries, top_k):
    """BEIR's exact search in numpy: longest text first (a stable sort), top_k + 1 by (score, position), the query's own id dropped"""
    ids = sorted(corpus, key=lambda c: len(corpus[c].get("title", "") + corpus[c].get("text", "")), reverse=True)
    emb = np.stack([_embed((corpus[c]["title"] + " " + corpus[c]["text"]).strip()) for c in ids]).astype(np.float64)
    want = {}
    for qid, text in queries.items():
        s = emb @ _embed(text).astype(np.float64)
        order = np.lexsort((np.arange(len(ids)), -s))[:top_k + 1]
        kept = [(ids[j], float(np.float32(s[j]))) for j in order if ids[j] != qid][:top_k]
        want[qid] = dict(kept)
    return want, ids


@pytest.fixture
def numpy_search(monkeypatch):
    NumpySearch.made = []
    monkeypatch.setattr(beir_exact, "StreamSearch", NumpySearch)
    return NumpySearch


@pytest.mark.parametrize("chunk", [7, 50, 1000])
def test_search_matches_the_restatement(numpy_search, chunk):
    corpus, queries = _data(50)
    model = FakeModel()
    es = beir_exact.ExactSearch(model, batch_size=16, corpus_chunk_size=chunk)
    got = es.search(corpus, queries, 10, "dot")
    want, ids = _restatement(corpus, queries, 10)
    assert got == want and got is es.results
    assert [list(got[q]) for q in queries] == [list(want[q]) for q in queries]          # best first
    for docid in list(corpus)[:2]:
        assert docid not in got[docid] and len(got[docid]) == 10
    (s,) = numpy_search.made
    assert s.k == 11 and s.closed
    assert s.adds == [(a, min(chunk, 50 - a)) for a in range(0, 50, chunk)]
    assert model.query_calls == [(list(queries.values()), 16)]
    fed = [t for texts, bs in model.corpus_calls for t in texts]
    assert fed == [(corpus[c]["title"] + " " + corpus[c]["text"]).strip() for c in ids] and all(bs == 16 for _, bs in model.corpus_calls)
    lengths = [len(corpus[c]["title"] + corpus[c]["text"]) for c in ids]
    assert lengths == sorted(lengths, reverse=True) and len(set(lengths)) < len(lengths)     # longest first, and the order of equal lengths was tested


def test_fewer_documents_than_top_k(numpy_search):
    corpus, queries = _data(5)
    got = beir_exact.ExactSearch(FakeModel(), corpus_chunk_size=2).search(corpus, queries, 10)
    want, _ = _restatement(corpus, queries, 10)
    assert got == want
    assert all(len(got[q]) == (4 if q in corpus else 5) for q in queries)


def test_arguments():
    es = beir_exact.ExactSearch(FakeModel())
    assert (es.batch_size, es.corpus_chunk_size) == (128, 50000)
    corpus, queries = _data(5)
    for fn in ("cos_sim", "cosine", None):
        with pytest.raises(ValueError, match="score_function"):
            es.search(corpus, queries, 10, fn)
    with pytest.raises(ValueError, match="top_k"):
        es.search(corpus, queries, 0)
    with pytest.raises(ValueError, match="corpus_chunk_size"):
        beir_exact.ExactSearch(FakeModel(), corpus_chunk_size=0)
    assert es.search({}, queries, 10) == {q: {} for q in queries} and es.search(corpus, {}, 10) == {}
