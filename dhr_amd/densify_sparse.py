"""Sparse term-weight vectors -> DLR index records on the fused HIP op `dhr_densify_sparse`: the `densify/` package of the reference
(densify/densify_corpus.py:29-93, densify/densify_query.py), the producer of its BM25, DeepImpact, uniCOIL and SPLADE indexes.

Two levels.  `densify_vectors` / `densify_vectors_into` take a whole block of vectors as CSR (indptr, term ids, weights) and make one library
call: numpy arrays (host memory, staged through the device, complete on return) or torch tensors (CUDA tensors are processed in place: the op is
enqueued on torch's current stream and the call does not wait for it).  `densify` and `vectorize_and_densify` carry the reference's names,
arguments, returns, printed totals, KeyError for an unknown term and the protocol-4 pickle [value, index, ids]; the second reads its files in
blocks of documents and makes one library call per block.

The fold is the reference's, entry by entry in the order given (include/dhr_hip.h), so the records are bit-identical to what the reference
leaves under NumPy >= 2.  There is no CPU implementation here: without the HIP library / a GPU the calls raise."""
from __future__ import annotations

import gzip
import json
import logging
import pickle

import numpy as np

from . import _lib
from . import _marshal as M

logger = logging.getLogger(__name__)

omission_num = {'bm25': 472, 'deepimpact': 502, 'unicoil': 570, 'splade': 570}
whole_word_matching = {'bm25': True, 'deepimpact': True, 'unicoil': False, 'splade': False}

MAX_DIMS = 8192
BLOCK_DOCS = 8192                       # documents per library call of vectorize_and_densify
_GROUP_LIMIT = {"int8": 127, "uint8": 255, "int16": 32767}


def _check(indptr, ids, weights, dims, omission):
    """the wrappers' own errors, raised before the library is touched -> (batch, nnz)"""
    if len(indptr.shape) != 1 or len(ids.shape) != 1 or len(weights.shape) != 1:
        raise ValueError("indptr, ids and weights must be 1-D (CSR)")
    if int(indptr.shape[0]) < 1:
        raise ValueError("indptr needs batch + 1 entries")
    if int(ids.shape[0]) != int(weights.shape[0]):
        raise ValueError("ids and weights must have the same length, got {} and {}".format(int(ids.shape[0]), int(weights.shape[0])))
    if dims <= 0 or dims > MAX_DIMS:
        raise ValueError("dims must be in [1, {}], got {}".format(MAX_DIMS, dims))
    if omission < 0:
        raise ValueError("omission must not be negative, got {}".format(omission))
    kinds = {(M.is_np(a), M.mem_kind(a), M.device(a)) for a in (indptr, ids, weights)}
    if len(kinds) != 1:
        raise ValueError("indptr, ids and weights must be all numpy arrays or all tensors on one device")
    if "int" not in M.dtype_name(indptr) or "int" not in M.dtype_name(ids):
        raise TypeError("indptr and ids must be integer arrays")
    return int(indptr.shape[0]) - 1, int(ids.shape[0])


def _half_or_float(weights):
    """fp16 and fp32 weights as they are; every other dtype of a numpy array is rounded to fp16 HERE, in one step (the reference assigns a Python
    float into a float16 array: one rounding; a detour through fp32 can round twice).  torch has no single-step float64 -> float16 cast."""
    name = M.dtype_name(weights)
    if name in M.FLOATS:
        return weights
    if M.is_np(weights):
        with np.errstate(over="ignore"):
            return weights.astype(np.float16)
    raise TypeError("tensor weights must be float16 or float32, got {} (round float64 weights on the host: numpy float64 -> float16 is one step)".format(name))


def _contig(a):
    return np.ascontiguousarray(a) if M.is_np(a) else a.contiguous()


def _run(indptr, ids, weights, dims, omission, vocab, value_out, index_out, collisions):
    idx_name = M.dtype_name(index_out)
    if idx_name not in _GROUP_LIMIT:
        raise TypeError("index_out must be int8, uint8 or int16, got {}".format(idx_name))
    if M.dtype_name(value_out) not in M.FLOATS:
        raise TypeError("value_out must be float16 or float32, got {}".format(M.dtype_name(value_out)))
    batch, nnz = int(indptr.shape[0]) - 1, int(ids.shape[0])
    limit = _GROUP_LIMIT[idx_name]
    if vocab is None:
        # every id whose group fits the index dtype; what lies beyond is refused here for host arrays (the reference raises OverflowError when it
        # meets such a term) and skipped by the kernel for device arrays, which are not read back
        vocab = omission + dims * (limit + 1)
        if M.is_np(ids) and nnz and (int(ids.max()) - omission) // dims > limit:
            raise OverflowError("term id {} gives group {}, out of bounds for {}".format(int(ids.max()), (int(ids.max()) - omission) // dims, idx_name))
    for out in (value_out, index_out, collisions):
        if (M.is_np(out), M.mem_kind(out), M.device(out)) != (M.is_np(ids), M.mem_kind(ids), M.device(ids)):
            raise ValueError("inputs and outputs must live in the same memory (all numpy, or all tensors on one device)")
    indptr, ids, weights = _contig(M.cast(indptr, "int64")), _contig(ids if M.dtype_name(ids) in ("int32", "int64") else M.cast(ids, "int64")), _contig(weights)
    p_v, ld_v, kind = _lib._ptr_ld(value_out)
    p_i, ld_i, _ = _lib._ptr_ld(index_out)
    lib = _lib.load()
    _lib.check(lib.dhr_densify_sparse(M.device(ids), kind, M.data_ptr(indptr), M.data_ptr(ids), ids.itemsize if M.is_np(ids) else ids.element_size(),
                                      M.data_ptr(weights), _lib._val_code(weights), nnz, batch, int(vocab), omission, dims, p_v, _lib._val_code(value_out),
                                      ld_v, p_i, _lib.idx_code(index_out.dtype), ld_i, M.data_ptr(collisions), M.stream(ids)), "dhr_densify_sparse")


def densify_vectors(indptr, ids, weights, dims: int = 768, omission: int = 570, whole_word_matching: bool = False, vocab=None):
    """A block of sparse vectors in CSR form -> (value [batch, dims] float16, index [batch, dims] int16 if whole_word_matching else int8,
    collisions [batch] int32).  Vector b holds the entries [indptr[b], indptr[b + 1]) of ids (term ids, int32 or int64) and weights (float16 or
    float32; any other numpy dtype is rounded to float16 on the host in one step).  Entries with an id below `omission` are skipped, the others
    are folded in the order given, as the reference's `densify` does.  numpy in -> numpy out; CUDA tensors in -> tensors out, enqueued on
    torch's current stream without waiting.

    `vocab` (optional) is the size of the vocabulary: ids at or beyond it are skipped.  Without it every id whose group fits the index dtype is
    taken; numpy ids beyond that raise OverflowError, as the reference does when it meets such a term."""
    dims, omission = int(dims), int(omission)
    batch, _ = _check(indptr, ids, weights, dims, omission)
    weights = _half_or_float(weights)
    value = M.empty(ids, (batch, dims), "float16")
    index = M.empty(ids, (batch, dims), "int16" if whole_word_matching else "int8")
    collisions = M.empty(ids, (batch,), "int32")
    if batch:
        _run(indptr, ids, weights, dims, omission, vocab, value, index, collisions)
    return value, index, collisions


def densify_vectors_into(indptr, ids, weights, value_out, index_out, dims: int = 768, omission: int = 570, vocab=None):
    """The same into the first `dims` columns of record arrays the caller owns (rows of width dims + cls_dim, say): value_out [batch, >= dims]
    float16 or float32, index_out [batch, >= dims] int8, uint8 or int16, the last dimension contiguous.  Columns beyond `dims` are not touched.
    -> (value_out, index_out, collisions [batch] int32)."""
    dims, omission = int(dims), int(omission)
    batch, _ = _check(indptr, ids, weights, dims, omission)
    weights = _half_or_float(weights)
    if len(value_out.shape) != 2 or len(index_out.shape) != 2 or int(value_out.shape[0]) != batch or int(index_out.shape[0]) != batch or \
            int(value_out.shape[1]) < dims or int(index_out.shape[1]) < dims:
        raise ValueError("output arrays do not match the batch / dims")
    collisions = M.empty(ids, (batch,), "int32")
    if batch:
        _run(indptr, ids, weights, dims, omission, vocab, value_out, index_out, collisions)
    return value_out, index_out, collisions


# ------------------------------------------------------------------------------------------ the reference's functions
def _csr(vectors, token2id):
    """[{term: weight}, ...] -> (indptr int64, ids int64, weights float16); KeyError for a term that token2id does not know"""
    indptr = np.zeros(len(vectors) + 1, np.int64)
    ids, weights = [], []
    for n, vector in enumerate(vectors):
        for token, weight in vector.items():
            ids.append(token2id[token])
            weights.append(weight)
        indptr[n + 1] = len(ids)
    with np.errstate(over="ignore"):
        return indptr, np.asarray(ids, np.int64).reshape(-1), np.asarray(weights, np.float64).reshape(-1).astype(np.float16)


def densify(data, dim, whole_word_matching, token2id, args):
    """densify_corpus.py:29-52 for one vector: data['vector'] is {term: weight}, args.model names the omission number.
    -> (value [dim] float16, index [dim] int16 / int8, collision_num)."""
    indptr, ids, weights = _csr([data['vector']], token2id)
    value, index, collisions = densify_vectors(indptr, ids, weights, dim, omission_num[args.model], whole_word_matching)
    return value[0], index[0], int(collisions[0])


def _open(file, file_type):
    return gzip.open(file, "rb") if file_type == 'jsonl.gz' else open(file, 'r')


def vectorize_and_densify(files, file_type, dim, whole_word_matching, token2id, output_path, args):
    """densify_corpus.py:55-93: every line of `files` is {"id": ..., "vector": {term: weight}}; writes [value, index, docids] to output_path
    (pickle protocol 4) and prints the collision total.  The lines are read in blocks of BLOCK_DOCS documents, one library call per block,
    each writing its rows of the two arrays in place."""
    data_num = 0
    logger.info('count line number')
    for file in files:
        with _open(file, file_type) as f:
            for _ in f:
                data_num += 1
    logger.info('initialize numpy array with {}X{}'.format(data_num, dim))
    value_encoded = np.zeros((data_num, dim), dtype=np.float16)
    index_encoded = np.zeros((data_num, dim), dtype=np.int16 if whole_word_matching else np.int8)
    docids, total_collision_num, counter = [], 0, 0

    def flush(vectors):
        nonlocal total_collision_num, counter
        if not vectors:
            return
        indptr, ids, weights = _csr(vectors, token2id)
        rows = slice(counter, counter + len(vectors))
        _, _, collisions = densify_vectors_into(indptr, ids, weights, value_encoded[rows], index_encoded[rows], dim, omission_num[args.model])
        total_collision_num += int(collisions.sum(dtype=np.int64))
        counter += len(vectors)

    block = []
    for file in files:
        with _open(file, file_type) as f:
            for line in f:
                data = json.loads(line)
                docids.append(data['id'])
                block.append(data['vector'])
                if len(block) == BLOCK_DOCS:
                    flush(block)
                    block = []
    flush(block)
    print('Total {} collisions with {} passages'.format(total_collision_num, data_num))
    with open(output_path, 'wb') as f_out:
        pickle.dump([value_encoded, index_encoded, docids], f_out, protocol=4)


def read_vocab_file(path):
    """one term per line, id = line number (from 0) -> {term: id}"""
    with open(path, 'r', encoding='utf-8') as f:
        return {line.rstrip('\n'): n for n, line in enumerate(f)}


# ------------------------------------------------------------------------------------------ the command lines
def _token2id(args, query: bool):
    """-> (token2id, analyzer or None, query_encoder or None).  --vocab_file needs nothing else; without it the reference's loaders are
    imported here, when they are needed: a Lucene index reader for bm25 / deepimpact, a transformers tokenizer for unicoil / splade."""
    if args.model not in omission_num:
        raise ValueError('We cannot handle you input --model')
    if args.vocab_file:
        return read_vocab_file(args.vocab_file), None, None
    analyzer = encoder = None
    if args.model in ('bm25', 'deepimpact'):
        from pyserini.index import IndexReader
        token2id = {token.term: idx for idx, token in enumerate(IndexReader(args.tokenizer).terms())}
        if query and args.model == 'bm25':
            from pyserini.analysis import Analyzer, get_lucene_analyzer
            analyzer = Analyzer(get_lucene_analyzer())
    else:
        from transformers import AutoTokenizer
        token2id = AutoTokenizer.from_pretrained(args.tokenizer).vocab
        if query:
            if args.model != 'unicoil':
                raise ValueError('splade queries need their vectors: encode them and densify the vector files, or give --vocab_file')
            from pyserini.encode import UniCoilQueryEncoder
            encoder = UniCoilQueryEncoder('castorini/unicoil-msmarco-passage')
    return token2id, analyzer, encoder


def _mkdirs(*paths):
    import os
    for p in paths:
        if not os.path.exists(p):
            os.mkdir(p)


def get_files(directory):
    import glob
    import os
    for pattern, file_type in (('*.json', 'json'), ('*.jsonl.gz', 'jsonl.gz')):
        files = glob.glob(os.path.join(directory, pattern))
        if files:
            return files, file_type
    raise ValueError('There is no json or jsonl.gz files in {}'.format(directory))


def corpus_main(argv=None):
    """python -m densify.densify_corpus: the reference's flags and output files (<output_dir>/encoding/<prefix>.split<i>.pt, the files dealt to
    --num_workers splits as the reference deals them), plus --vocab_file.  The splits run one after the other in this process: the device does
    the work that the reference spreads over one Python process per file."""
    import argparse
    import os
    parser = argparse.ArgumentParser(description='Densify corpus')
    parser.add_argument('--model', required=True, help='bm25, deepimpact, unicoil or splade')
    parser.add_argument('--tokenizer', required=False, default="bert-base-uncased", help='anserini index path or transformer tokenizer')
    parser.add_argument('--vocab_file', required=False, default=None, help='one term per line, id = line number; replaces --tokenizer')
    parser.add_argument('--vector_dir', required=True, help='directory with json files')
    parser.add_argument('--output_dir', required=True, help='output pickle directory')
    parser.add_argument('--output_dims', type=int, required=False, default=768)
    parser.add_argument('--num_workers', type=int, required=False, default=None)
    parser.add_argument('--prefix', required=True, help='index name prefix')
    args = parser.parse_args(argv)
    token2id, _, _ = _token2id(args, query=False)
    out_dir = os.path.join(args.output_dir, 'encoding')
    _mkdirs(args.output_dir, out_dir)
    files, file_type = get_files(args.vector_dir)
    if args.num_workers is None:
        args.num_workers, per_split = len(files), 1
    else:
        per_split = len(files) // args.num_workers
        if len(files) % args.num_workers:
            args.num_workers += 1
    for i in range(args.num_workers):
        start = i * per_split
        part = files[start:] if i == args.num_workers - 1 else files[start:start + per_split]
        vectorize_and_densify(part, file_type, args.output_dims, whole_word_matching[args.model], token2id,
                              os.path.join(out_dir, "{}.split{}.pt".format(args.prefix, i)), args)


def query_main(argv=None):
    """python -m densify.densify_query: a tsv of (qid, query) -> <output_dir>/encoding/queries/<prefix>.<query file with tsv -> pt>, the
    pickle [value float16, index int16, qids].  bm25 / deepimpact queries weigh each term by its frequency; with --vocab_file the terms are
    the space-separated words of the query, for every model."""
    import argparse
    import os
    from collections import defaultdict
    parser = argparse.ArgumentParser(description='Densify queries')
    parser.add_argument('--model', required=True, help='bm25, deepimpact, unicoil or splade')
    parser.add_argument('--tokenizer', required=False, default="bert-base-uncased", help='anserini index path or transformer tokenizer')
    parser.add_argument('--vocab_file', required=False, default=None, help='one term per line, id = line number; replaces --tokenizer')
    parser.add_argument('--query_path', required=True, help='query tsv file')
    parser.add_argument('--output_dims', type=int, required=False, default=768)
    parser.add_argument('--output_dir', required=True, help='output pickle directory')
    parser.add_argument('--prefix', required=True, help='index name prefix')
    args = parser.parse_args(argv)
    args.model = args.model.lower()
    token2id, analyzer, encoder = _token2id(args, query=True)
    out_dir = os.path.join(args.output_dir, 'encoding', 'queries')
    _mkdirs(args.output_dir, os.path.join(args.output_dir, 'encoding'), out_dir)
    qids, vectors = [], []
    with open(args.query_path, 'r') as f:
        for line in f:
            qid, query = line.strip().split('\t')
            if encoder is not None:
                vector = encoder.encode(query)
            else:
                vector = defaultdict(int)                     # term frequency as the weight
                for term in (analyzer.analyze(query) if analyzer is not None else query.split(' ')):
                    vector[term] += 1
            qids.append(qid)
            vectors.append(vector)
    print('initialize numpy array with {}X{}'.format(len(qids), args.output_dims))
    indptr, ids, weights = _csr(vectors, token2id)
    value, index, collisions = densify_vectors(indptr, ids, weights, args.output_dims, omission_num[args.model], whole_word_matching[args.model])
    print('Total {} collisions with {} queries'.format(int(collisions.sum(dtype=np.int64)), len(qids)))
    name = args.prefix + '.' + args.query_path.split('/')[-1].replace('tsv', 'pt')
    with open(os.path.join(out_dir, name), 'wb') as f_out:
        pickle.dump([value, index.astype(np.int16), qids], f_out, protocol=4)
