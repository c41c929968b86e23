#!/usr/bin/env python
"""Golden vectors for the differentiable MaxSim scores (dhr_amd/maxsim_scores.py): runs the REFERENCE's own code -- ColBERT.listwise_maxsim and
ColBERT.pairwise_maxsim called unbound on a stub `self` (model_args.projection_out_dim, data_args.train_n_passages), and the non-training,
non-teacher branch of ColBERT.forward (modeling.py:188-190) on a stub whose encoders return the given token vectors and zero CLS vectors --
on fp32 CPU leaves, then .backward(G) with a seeded G.  Stores inputs, G, scores and both gradients.

Every input value is a multiple of 2^-3 in [-2, 2] and G a multiple of 2^-4 in [-2, 2]: with D <= 768 every product, score and gradient is
exact in fp32 (and the inputs in fp16), so any correct implementation reproduces the file bit for bit, ties included.  Inputs are stored as
int8 (value * 8), gradients as int16 (value * 128; the generator asserts that nothing is lost): the file stays below 512 KB.
Run in the build container only (the reference checkout is not part of the repository):  python tests/golden/make_golden_maxsim.py"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
from tevatron.ColBERT import modeling as CM  # noqa: E402

rng = np.random.default_rng(20261017)
out = {}
names = []


LEVELS = np.array([-16, -6, -3, -1, 0, 1, 3, 6, 16], np.int8)       # x 2^-3: nine levels keep the file small and make exact ties common


def tokens(n, L, D):
    return LEVELS[rng.integers(0, len(LEVELS), (n, L, D))]


def seeded_g(shape):
    return (rng.integers(-32, 33, shape) / 16.0).astype(np.float32)


def run(fn, q8, p8):
    """-> (scores, G, dL/dq, dL/dp) of scores = fn(q, p) on fp32 CPU leaves"""
    tq = torch.from_numpy(q8.astype(np.float32) / 8).requires_grad_(True)
    tp = torch.from_numpy(p8.astype(np.float32) / 8).requires_grad_(True)
    s = fn(tq, tp)
    g = seeded_g(tuple(s.shape))
    s.backward(torch.from_numpy(g))
    return s.detach().numpy(), g, tq.grad.numpy(), tp.grad.numpy()


def case(name, q8, p8, n):
    """listwise, pairwise (A x n) and paired (q against the first passage of each query) on one pair of inputs"""
    A, Lq, D = q8.shape
    B, Lp, _ = p8.shape
    assert B == A * n
    stub = types.SimpleNamespace(model_args=types.SimpleNamespace(projection_out_dim=D), data_args=types.SimpleNamespace(train_n_passages=n))
    names.append(name)
    out[name + "_q"], out[name + "_p"] = q8, p8
    out[name + "_geom"] = np.array([A, B, n, Lq, Lp, D])

    def paired(a, b):
        cls = lambda t: torch.zeros(t.shape[0], 1, D)  # noqa: E731
        fwd = types.SimpleNamespace(training=False, train_args=types.SimpleNamespace(negatives_x_device=False), model_args=stub.model_args,
                                    encode_query=lambda _: (cls(a), a), encode_passage=lambda _: (cls(b), b))
        return CM.ColBERT.forward(fwd, {"input_ids": 1}, {"input_ids": 1}).scores
    modes = {"list": (lambda a, b: CM.ColBERT.listwise_maxsim(stub, a, b), p8),
             "pair": (lambda a, b: CM.ColBERT.pairwise_maxsim(stub, a, b), p8),
             "one": (paired, np.ascontiguousarray(p8[::n]))}
    for mode, (fn, pp) in modes.items():
        s, g, gq, gp = run(fn, q8, pp)
        gq128, gp128 = np.rint(gq * 128).astype(np.int16), np.rint(gp * 128).astype(np.int16)
        assert np.array_equal(gq128 / 128.0, gq) and np.array_equal(gp128 / 128.0, gp)
        out[f"{name}_{mode}_scores"], out[f"{name}_{mode}_G"], out[f"{name}_{mode}_gq"], out[f"{name}_{mode}_gp"] = s, g, gq128, gp128


def pattern(D):
    return (rng.integers(0, 2, D) * 2 - 1).astype(np.int8) * 16          # +-2 in every dimension


# the recipe's token counts: 31 x 149, D = 128; the last 9 passage tokens and the last 5 tokens of query 1 are padding (zero vectors)
q, p = tokens(4, 31, 128), tokens(12, 149, 128)
p[:, 140:] = 0
q[1, 26:] = 0
s = pattern(128)
p[1, 2] = p[1, 5] = s                   # two equal passage tokens that win (similarity 512): token 2 takes the gradient
q[0, 3] = s
p[6, :140, 0] = 16                      # every real token of passage 6 (query 2's first) has +2 in dimension 0 ...
q[2, 7] = 0
q[2, 7, 0] = -16                        # ... so this query token is at -4 against all of them: the first padded token (140) wins with 0
case("base", q, p, 3)
# the CLS call: one token on both sides
case("cls", tokens(4, 1, 128), tokens(12, 1, 128), 3)
# rows that are no multiple of 16 bytes
case("d20", tokens(3, 5, 20), tokens(6, 7, 20), 2)
# one token past a 32-block on both sides; winners at the last passage token (64) and at the first (0)
q, p = tokens(2, 33, 32), tokens(4, 65, 32)
s, t = pattern(32), pattern(32)
p[0, 64] = s
q[0, 32] = q[0, 0] = s
p[1, 0] = t
q[0, 5] = q[1, 32] = t
p[2, 0] = p[2, 64] = s                  # equal at both ends of passage 2: token 0 wins
case("edge", q, p, 2)
# exactly one 32-block of passage tokens
case("lp32", tokens(2, 8, 32), tokens(4, 32, 32), 2)
# D = 768: the K loop
case("d768", tokens(2, 4, 768), tokens(4, 40, 768), 2)
# one query: pairwise returns [n]
case("a1", tokens(1, 6, 16), tokens(3, 9, 16), 3)
# one passage per query: pairwise returns [A]
case("n1", tokens(4, 6, 16), tokens(4, 9, 16), 1)

# the exception types of the shape mismatches
stub = types.SimpleNamespace(model_args=types.SimpleNamespace(projection_out_dim=16), data_args=types.SimpleNamespace(train_n_passages=3))
z = lambda n, L, D=16: torch.zeros(n, L, D)  # noqa: E731
errs = []
for label, fn in (("listwise: 16 and 20 dims", lambda: CM.ColBERT.listwise_maxsim(stub, z(2, 5), z(6, 7, 20))),
                  ("pairwise: 5 passage rows for 2 x 3", lambda: CM.ColBERT.pairwise_maxsim(stub, z(2, 5), z(5, 7)))):
    try:
        fn()
        errs.append(label + " | | ")
    except (ValueError, RuntimeError) as e:
        errs.append(label + " | " + type(e).__name__ + " | " + str(e).split("\n")[0])
out["errors"] = np.array(errs)
out["names"] = np.array(names)
path = os.path.join(HERE, "maxsim_golden.npz")
np.savez_compressed(path, **out)
assert os.path.getsize(path) < 512 * 1024
print(os.path.getsize(path), "bytes;", {k: getattr(v, "shape", None) for k, v in out.items() if k.endswith("_scores")})
print("\n".join(errs))
