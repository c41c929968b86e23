#!/usr/bin/env python
"""Golden vectors for the differentiable gated-inner-product scores (dhr_amd/gip_scores.py): runs the REFERENCE's own code --
DHRModel.listwise_gip_scores and DHRModel.pairwise_gip_scores called unbound on a stub `self` (model_args.dlr_out_dim,
data_args.train_n_passages), and the non-training branch of DHRModel.forward (modeling.py:214-218) on a stub whose encoders return the
given lexical reps, lamb = 0 -- on fp32 CPU tensors with requires_grad, then .backward(G) with a seeded G.  Stores inputs, G, scores and both
gradients.  The reference's methods never pass remove_dims, so densify runs with its default 570: the small cases use vocabularies of
570 + groups * dims.  Values are multiples of 2^-6 and G of 2^-4 (the file compresses; no gradient leaves fp16's normal range).
Run in the build container only (the reference checkout is not part of the repository):  python tests/golden/make_golden_gip_scores.py"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
from tevatron.DHR import modeling as DM  # noqa: E402

rng = np.random.default_rng(20261017)
REMOVE = 570
out = {}
names = []


def reps(rows, dims, groups, density, negative=False):
    """[rows, 570 + groups * dims] fp32, multiples of 2^-6; `density` of the entries non-zero (the first 570 columns too: they must be ignored)"""
    V = REMOVE + groups * dims
    x = np.round(rng.uniform(0.05, 3.0, (rows, V)) * 64) / 64
    if negative:
        x = x * rng.choice([-1.0, 1.0], (rows, V))
    return (x * (rng.random((rows, V)) < density)).astype(np.float32)


def seeded_g(shape):
    g = np.round(rng.uniform(-2.0, 2.0, shape) * 16) / 16
    g[g == 0] = 0.0625
    return g.astype(np.float32)


def run(fn, q, p):
    """-> (scores, G, dL/dq, dL/dp) of scores = fn(q, p) on fp32 CPU leaves"""
    tq, tp = torch.from_numpy(q).clone().requires_grad_(True), torch.from_numpy(p).clone().requires_grad_(True)
    s = fn(tq, tp)
    g = seeded_g(tuple(s.shape))
    s.backward(torch.from_numpy(g))
    return s.detach().numpy(), g, tq.grad.numpy(), tp.grad.numpy()


def case(name, q, p, dims, bsz, n):
    """listwise (effective_bsz = bsz), pairwise (bsz x n) and paired (q against the first passage of each query) on one pair of inputs"""
    stub = types.SimpleNamespace(model_args=types.SimpleNamespace(dlr_out_dim=dims), data_args=types.SimpleNamespace(train_n_passages=n))
    assert p.shape[0] == bsz * n and q.shape[0] == bsz
    names.append(name)
    out[name + "_q"], out[name + "_p"] = q, p
    out[name + "_geom"] = np.array([dims, REMOVE, bsz, n])
    modes = {"list": (lambda a, b: DM.DHRModel.listwise_gip_scores(stub, a, b, bsz), p),
             "pair": (lambda a, b: DM.DHRModel.pairwise_gip_scores(stub, a, b, bsz), p)}

    def paired(a, b):
        fwd = types.SimpleNamespace(training=False, lamb=0, model_args=stub.model_args,
                                    encode_query=lambda _: (a, torch.zeros(a.shape[0], 1)), encode_passage=lambda _: (b, torch.zeros(b.shape[0], 1)))
        return DM.DHRModel.forward(fwd, {"input_ids": 1}, {"input_ids": 1}).scores
    modes["one"] = (paired, np.ascontiguousarray(p[::n]))
    for mode, (fn, pp) in modes.items():
        s, g, gq, gp = run(fn, q, pp)
        out[f"{name}_{mode}_scores"], out[f"{name}_{mode}_G"], out[f"{name}_{mode}_gq"], out[f"{name}_{mode}_gp"] = s, g, gq, gp


# production vocabulary 30522 / 768 / 570 (39 groups), sparse rows; an equal maximum in two groups of one slice on both sides
q, p = reps(3, 768, 39, 0.01), reps(6, 768, 39, 0.02)
q[0, REMOVE + 5] = q[0, REMOVE + 768 * 7 + 5] = 3.5
p[1, REMOVE + 5] = p[1, REMOVE + 768 * 2 + 5] = 3.25
p[4, REMOVE + 5] = 2.0
q[:, :REMOVE] = 4.0                                                # the removed columns never count and get a zero gradient
case("prod", q, p, 768, 3, 2)

# small vocabulary with designed ties: dims 8, 5 groups, V = 610
q, p = reps(4, 8, 5, 0.5), reps(12, 8, 5, 0.5)
q[0, REMOVE + 1] = q[0, REMOVE + 8 * 3 + 1] = 3.5                  # equal maxima in groups 0 and 3: group 0 wins and gets the gradient
p[0, REMOVE + 1] = 1.5
p[0, REMOVE + 8 + 1] = p[0, REMOVE + 8 * 4 + 1] = 3.25             # equal maxima in groups 1 and 4 on the passage side
p[1, REMOVE + 8 * 2 + 1] = p[1, REMOVE + 8 * 3 + 1] = 3.75
for g in range(5):                                                 # all-zero slices on both sides: they MATCH at group 0 (products are zero)
    q[1, REMOVE + 8 * g + 2] = 0.0
    p[3, REMOVE + 8 * g + 2] = p[4, REMOVE + 8 * g + 2] = 0.0
q[2] = 0.0                                                         # a whole row of zeros: every index 0, gradient at columns 570 .. 577
p[5] = 0.0
case("ties", q, p, 8, 4, 3)

# negative values (a slice whose maximum is negative still matches and multiplies)
q, p = reps(3, 8, 5, 1.0, negative=True), reps(6, 8, 5, 1.0, negative=True)
for g in range(5):
    q[0, REMOVE + 8 * g + 3] = -0.25 * (g + 1)
    p[0, REMOVE + 8 * g + 3] = -0.5 * (6 - g)
case("neg", q, p, 8, 3, 2)

# effective_bsz = 1: the reference's squeeze returns [P]
case("bsz1", reps(1, 8, 5, 0.6), reps(5, 8, 5, 0.6), 8, 1, 5)
# one passage per query: pairwise returns [bsz]
case("n1", reps(4, 8, 5, 0.6), reps(4, 8, 5, 0.6), 8, 4, 1)
# more than 256 groups (int16 indices): dims 8, 300 groups, V = 2970
q, p = reps(3, 8, 300, 0.05), reps(6, 8, 300, 0.05)
q[0, REMOVE + 8 * 299 + 4] = p[2, REMOVE + 8 * 299 + 4] = 3.5      # the last group on both sides
q[1, REMOVE + 8 * 257 + 6] = p[3, REMOVE + 8 * 257 + 6] = 3.25     # a group beyond uint8 that matches; 257 - 256 = 1 must not
p[2, REMOVE + 8 * 1 + 6] = 3.0
case("wide", q, p, 8, 3, 2)

# the exception types of the shape mismatches and of densify
stub = types.SimpleNamespace(model_args=types.SimpleNamespace(dlr_out_dim=8), data_args=types.SimpleNamespace(train_n_passages=3))
z = lambda rows, V=610: torch.zeros(rows, V)  # noqa: E731
errs = []
for label, fn in (("listwise: 4 query rows, effective_bsz 2", lambda: DM.DHRModel.listwise_gip_scores(stub, z(4), z(6), 2)),
                  ("listwise: 2 query rows, effective_bsz 4", lambda: DM.DHRModel.listwise_gip_scores(stub, z(2), z(6), 4)),
                  ("pairwise: 5 passage rows for 2 x 3", lambda: DM.DHRModel.pairwise_gip_scores(stub, z(2), z(5), 2)),
                  ("pairwise: 12 passage rows for 2 x 3", lambda: DM.DHRModel.pairwise_gip_scores(stub, z(2), z(12), 2)),
                  ("pairwise: 3 query rows, effective_bsz 2", lambda: DM.DHRModel.pairwise_gip_scores(stub, z(3), z(6), 2)),
                  ("listwise: vocabulary 611", lambda: DM.DHRModel.listwise_gip_scores(stub, z(2, 611), z(6), 2)),
                  ("listwise: passages of vocabulary 611", lambda: DM.DHRModel.listwise_gip_scores(stub, z(2), z(6, 611), 2)),
                  ("pairwise: 3-dimensional reps", lambda: DM.DHRModel.pairwise_gip_scores(stub, torch.zeros(2, 1, 610), z(6), 2))):
    try:
        fn()
        errs.append(label + " | | ")
    except (ValueError, RuntimeError) as e:
        errs.append(label + " | " + type(e).__name__ + " | " + str(e).split("\n")[0])
out["errors"] = np.array(errs)
out["names"] = np.array(names)
path = os.path.join(HERE, "gip_scores_golden.npz")
np.savez_compressed(path, **out)
print(os.path.getsize(path), "bytes;", {k: getattr(v, "shape", None) for k, v in out.items()})
print("\n".join(errs))
