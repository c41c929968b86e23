#!/usr/bin/env python
"""Golden vectors for the sparse densify (dhr_amd/densify_sparse.py, dhr_densify_sparse): runs the REFERENCE functions `densify` and
`vectorize_and_densify` of densify/densify_corpus.py on fixed inputs and stores inputs + outputs in densify_sparse_golden.npz.

    python tests/golden/make_golden_densify_sparse.py <root of the reference checkout>

The reference file is loaded by its path, with `pyserini.index` stubbed (it is imported at the top of the file and used only by main());
no package named `densify` is imported, since this repository has one of its own.  `value[s] < weight` compares a float16 scalar with a
Python number, which NumPy >= 2 does in float16 and NumPy 1 in float64: the fixture is only valid from NumPy 2 on, asserted below.

Layout of the fixture: case c has the entries [case_ptr[c], case_ptr[c + 1]) of `ids` (int64) and `weights` (float64: the Python number handed
to the reference, an int where `is_int[c]`), in the order the reference saw them; `omission`, `dims`, `wwm` (1: int16 index, 0: int8), `name`
per case; the outputs [out_ptr[c], out_ptr[c + 1]) of `value_bits` (the float16 bits as uint16) and `index` (int16 holds both dtypes);
`collisions` per case.  corpus_*: one JSONL vector file (bm25, dims 16), its vocabulary file (one term per line, id = line number) and what
vectorize_and_densify pickled for it."""
import importlib.util
import json
import os
import pickle
import sys
import tempfile
import types
import warnings

import numpy as np

assert int(np.__version__.split(".")[0]) >= 2, "the fold compares in float16 only under NumPy >= 2"
HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1]

stub = types.ModuleType("pyserini.index")
stub.IndexReader = None
sys.modules.setdefault("pyserini", types.ModuleType("pyserini"))
sys.modules["pyserini.index"] = stub
spec = importlib.util.spec_from_file_location("ref_densify_corpus", os.path.join(REF, "densify", "densify_corpus.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

LIMIT = {0: 127, 1: 32767}
rng = np.random.default_rng(20261021)
cases = []


def add(name, model, dims, ids, weights, is_int=False):
    wwm = int(ref.whole_word_matching[model])
    weights = [int(w) for w in weights] if is_int else [float(w) for w in weights]
    token2id = {"t%d" % n: int(t) for n, t in enumerate(ids)}
    data = {"vector": {"t%d" % n: w for n, w in enumerate(weights)}}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                   # "overflow encountered in cast" for the weight above 65 504
        value, index, coll = ref.densify(data, dims, bool(wwm), token2id, types.SimpleNamespace(model=model))
    cases.append(dict(name=name, omission=ref.omission_num[model], dims=dims, wwm=wwm, is_int=int(is_int), ids=np.asarray(ids, np.int64),
                      weights=np.asarray(weights, np.float64), value=value.view(np.uint16).copy(), index=index.astype(np.int16), coll=coll))


def top_id(model, dims, cap):
    """one past the largest id whose group fits the model's index dtype, at most cap"""
    return min(cap, ref.omission_num[model] + dims * (LIMIT[int(ref.whole_word_matching[model])] + 1))


for model in ("bm25", "deepimpact", "unicoil", "splade"):
    om = ref.omission_num[model]
    for dims in (8, 768):
        hi = top_id(model, dims, 2_000_000 if ref.whole_word_matching[model] else 30522)
        n = 60 if dims == 768 else 40
        ids = np.concatenate([rng.integers(0, om, 5), rng.integers(om, hi, n)])
        rng.shuffle(ids)
        add(f"{model}-d{dims}-weights", model, dims, ids, rng.uniform(0.05, 12.0, ids.size))          # BM25 / impact like weights
        add(f"{model}-d{dims}-tf", model, dims, ids, rng.integers(1, 5, ids.size), is_int=True)      # integer term frequencies
        signed = rng.choice([0.0, -0.0, -1.5, 2.25, 1e-9, -1e-9, 3.0, -3.0, 0.5], ids.size)
        add(f"{model}-d{dims}-signed", model, dims, ids, signed)                                    # zeros, -0.0, negatives, weights that round to 0
        add(f"{model}-d{dims}-empty", model, dims, [], [])
        add(f"{model}-d{dims}-all-omitted", model, dims, rng.integers(0, om, 7), rng.uniform(0.5, 2.0, 7))
        g = LIMIT[int(ref.whole_word_matching[model])] + 1
        one = om + 3 % dims + dims * rng.permutation(min(g, 100))                                    # every entry in one slice
        add(f"{model}-d{dims}-one-slice", model, dims, one, rng.uniform(0.05, 12.0, one.size))
        add(f"{model}-d{dims}-one-slice-signed", model, dims, one, rng.choice([0.0, -0.0, -2.0, -1.0, 1.0, 1e-9, 2.0], one.size))
        # ties that exist only after the rounding to float16: the first of a pair must keep the slice, in either order
        s0, s1, s2 = om, om + 1 % dims, om + 2 % dims
        for tag, (a, b) in (("near-one", (1.0002, 1.0004)), ("near-2048", (2048.4, 2049.0))):
            add(f"{model}-d{dims}-tie-{tag}", model, dims, [s0, s0 + dims, s1 + dims, s1], [a, b, a, b])
            add(f"{model}-d{dims}-tie-{tag}-reversed", model, dims, [s0, s0 + dims, s1 + dims, s1], [b, a, b, a])
        add(f"{model}-d{dims}-above-65504", model, dims, [s0, s0 + dims, s1, s1 + dims, s2 + dims, s2], [70000.0, 65504.0, 65504.0, 65520.0, 1e30, 1e30])
        add(f"{model}-d{dims}-negative-then-zero", model, dims, [s0, s0 + dims, s0 + 2 * dims, s1, s1 + dims], [-2.0, 0.0, -3.0, -0.0, 0.0])

out = {"numpy_version": np.array(np.__version__), "name": np.array([c["name"] for c in cases])}
for k in ("omission", "dims", "wwm", "is_int"):
    out[k] = np.array([c[k] for c in cases], np.int32)
out["collisions"] = np.array([c["coll"] for c in cases], np.int32)
out["case_ptr"] = np.concatenate([[0], np.cumsum([c["ids"].size for c in cases])]).astype(np.int64)
out["out_ptr"] = np.concatenate([[0], np.cumsum([c["dims"] for c in cases])]).astype(np.int64)
out["ids"] = np.concatenate([c["ids"] for c in cases])
out["weights"] = np.concatenate([c["weights"] for c in cases])
out["value_bits"] = np.concatenate([c["value"] for c in cases])
out["index"] = np.concatenate([c["index"] for c in cases])

# ---- the corpus: 40 lines of {"id", "vector"} over a vocabulary of 472 + 16 * 50 terms, an empty vector and a repeated-slice one among them
vocab = ["w%04d" % n for n in range(472 + 16 * 50)]
lines = []
for d in range(40):
    n = 0 if d == 7 else int(rng.integers(5, 40))
    terms = rng.choice(len(vocab), n, replace=False)
    lines.append(json.dumps({"id": "doc%d" % d, "vector": {vocab[t]: round(float(rng.uniform(0.1, 9.0)), 4) for t in terms}}))
jsonl = "\n".join(lines) + "\n"
with tempfile.TemporaryDirectory() as tmp:
    path, pt = os.path.join(tmp, "docs.json"), os.path.join(tmp, "out.pt")
    with open(path, "w") as f:
        f.write(jsonl)
    ref.vectorize_and_densify([path], "json", 16, True, {t: n for n, t in enumerate(vocab)}, pt, types.SimpleNamespace(model="bm25"))
    with open(pt, "rb") as f:
        value, index, docids = pickle.load(f)
out["corpus_jsonl"] = np.frombuffer(jsonl.encode(), np.uint8)
out["corpus_vocab"] = np.frombuffer(("\n".join(vocab) + "\n").encode(), np.uint8)
out["corpus_value_bits"], out["corpus_index"], out["corpus_docids"] = value.view(np.uint16), index, np.array(docids)
assert value.dtype == np.float16 and index.dtype == np.int16

np.savez_compressed(os.path.join(HERE, "densify_sparse_golden.npz"), **out)
print(len(cases), "cases;", os.path.getsize(os.path.join(HERE, "densify_sparse_golden.npz")), "bytes")
