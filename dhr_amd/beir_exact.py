"""`ExactSearch`: the retriever object that the reference's un-densified BEIR route hands to `beir.retrieval.evaluation.EvaluateRetrieval`
(`tevatron/datasets/beir/encode_and_retrieval.py`: `DRES(sentence_transformer)`, `score_function="dot"`), on `dhr_amd.stream_search.StreamSearch`.

    retriever = EvaluateRetrieval(ExactSearch(sentence_transformer), score_function="dot")
    results = retriever.retrieve(corpus, queries)            # {qid: {docid: score}}

The model protocol is the one `tevatron/datasets/beir/sentence_bert.py` implements: `encode_queries(list[str], batch_size=...)` and
`encode_corpus(list[{"title", "text"}], batch_size=...)`, each returning an [n, D] fp32 array (numpy, or a torch tensor: a CUDA tensor is read
where it is).  As in BEIR's exact search the corpus is taken longest text first (title + text, ties in the corpus' own order) and encoded
`corpus_chunk_size` documents at a time, `top_k + 1` results are asked for, a document whose id equals the query's id is dropped and `top_k` are
kept.  Scores are the exact inner products of stream_search.hip, not the fp32 `torch.mm` of the reference route: they differ from it by the
rounding of that product (tests/test_stream_search.py prints both errors), so documents whose scores are closer than that may change places.
`beir` itself is not a dependency and is not imported: parity with its `DenseRetrievalExactSearch` is unpinned, like the faiss row of the README."""
from __future__ import annotations

import numpy as np

from .stream_search import StreamSearch


class ExactSearch:
    def __init__(self, model, batch_size=128, corpus_chunk_size=50000):
        self.model, self.batch_size, self.corpus_chunk_size = model, int(batch_size), int(corpus_chunk_size)
        if self.corpus_chunk_size < 1:
            raise ValueError("corpus_chunk_size must be >= 1, got {}".format(corpus_chunk_size))
        self.results = {}

    def search(self, corpus, queries, top_k, score_function="dot", **kw):
        """corpus {docid: {"title", "text"}}, queries {qid: text} -> {qid: {docid: score}} with at most top_k documents per query"""
        if score_function != "dot":
            raise ValueError("score_function must be 'dot' (the un-densified route has no other), got {!r}".format(score_function))
        top_k = int(top_k)
        if top_k < 1:
            raise ValueError("top_k must be >= 1, got {}".format(top_k))
        query_ids = list(queries.keys())
        self.results = {qid: {} for qid in query_ids}
        if not query_ids or not corpus:
            return self.results
        q = self.model.encode_queries([queries[qid] for qid in query_ids], batch_size=self.batch_size)
        corpus_ids = sorted(corpus, key=lambda c: len(corpus[c].get("title", "") + corpus[c].get("text", "")), reverse=True)
        docs = [corpus[c] for c in corpus_ids]
        with StreamSearch(q, None, k=top_k + 1) as s:
            for start in range(0, len(docs), self.corpus_chunk_size):
                s.add(self.model.encode_corpus(docs[start:start + self.corpus_chunk_size], batch_size=self.batch_size), None, row_base=start)
            scores, rows = s.result()
        if not isinstance(scores, np.ndarray):
            scores, rows = scores.cpu().numpy(), rows.cpu().numpy()
        for i, qid in enumerate(query_ids):
            out = self.results[qid]
            for score, row in zip(scores[i].tolist(), rows[i].tolist()):
                if row < 0 or len(out) == top_k:
                    break
                if corpus_ids[row] != qid:
                    out[corpus_ids[row]] = score
        return self.results
