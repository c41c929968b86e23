#!/usr/bin/env python
"""Golden vectors for the fused training loss (dhr_amd/train_loss.py): runs the REFERENCE's own code -- DHRModel.forward and the Aggretriever
DenseModel.forward called unbound on a stub `self` (training, negatives_x_device = False, softmax, kl_loss, lamb, temperature, encoders that
return given leaves, a stub teacher whose call returns .scores, the class's own listwise_scores bound to the stub) -- on fp32 CPU leaves,
then loss.backward().  The Dense cross-entropy and ColBERT's padded-teacher KL are restated from Dense/modeling.py:134-140 and
ColBERT/modeling.py:146-160 with the same torch calls (their forwards need token encoders).

The query-side leaves are score-shaped [R, C] and the passage side is the identity, so the score matrices the forward builds ARE the leaves
(x @ I is exact) and the leaves' .grad is the gradient with respect to the score matrices.  For the Aggretriever model the leaves sit behind
cal_remove_dim(C) zero columns and agg_dim = C, semi_aggregate: one group, whose max is the identity.  Every score is a small integer
multiple of 2^-3.  Stores, per case: the score matrices, the teacher, lamb / temperature / weights / split / train_n_passages, the loss,
`scores` and the gradients, all as the reference's fp32 produced them.
Run in the build container only (the reference checkout is not part of the repository):  python tests/golden/make_golden_train_loss.py"""
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
from tevatron.Aggretriever import modeling as AM  # noqa: E402
from tevatron.Aggretriever.utils import cal_remove_dim  # noqa: E402
from tevatron.DHR import modeling as DM  # noqa: E402

rng = np.random.default_rng(20261019)
out, names = {}, []
SHAPES = ((2, 3), (3, 1), (8, 4))                  # (R, train_n_passages); C = R * n: no cross-device negatives


def grid(shape, span):
    return (rng.integers(-span, span + 1, shape) / 8.0).astype(np.float32)


class Teacher:
    def __init__(self, scores):
        self.scores = scores

    def eval(self):
        return self

    def __call__(self, query=None, passage=None, is_teacher=False):
        assert is_teacher
        return types.SimpleNamespace(scores=self.scores)


def stub(cls, R, n, tct, teacher, q_reps, p_reps, lamb, temperature, **model_args):
    s = types.SimpleNamespace(training=True, softmax=nn.Softmax(dim=-1), kl_loss=nn.KLDivLoss(reduction="batchmean"), lamb=lamb,
                              temperature=temperature, teacher_model=Teacher(teacher),
                              train_args=types.SimpleNamespace(negatives_x_device=False, per_device_train_batch_size=R),
                              data_args=types.SimpleNamespace(train_n_passages=n), model_args=types.SimpleNamespace(tct=tct, **model_args),
                              encode_query=lambda *_: q_reps, encode_passage=lambda *_: p_reps)
    s.listwise_scores = lambda q, p, bsz: cls.listwise_scores(s, q, p, bsz)
    return s


def keep(name, R, n, lex, sem, teacher, lamb, temperature, weights, split, loss, scores):
    loss.backward()
    names.append(name)
    out[name + "_lex"] = lex.detach().numpy()
    out[name + "_glex"] = lex.grad.numpy()
    if sem is not None:
        out[name + "_sem"], out[name + "_gsem"] = sem.detach().numpy(), sem.grad.numpy()
    if teacher is not None:
        out[name + "_teacher"] = teacher.numpy()
    out[name + "_loss"], out[name + "_scores"] = loss.detach().numpy(), scores.detach().numpy()
    out[name + "_cfg"] = np.array([R, n, lamb, temperature, *weights, *split], np.float64)


def leaf(a):
    return torch.from_numpy(a).requires_grad_(True)


D, H = (1.0, 0.5, 0.5), (1.0, 0.0, 0.0)
SPLIT = (1.0, 0.75, 0.25)
for R, n in SHAPES:
    C = R * n
    eye = torch.eye(C)
    tag = f"{R}x{n}"
    # DHRModel.forward: --tct, --tct with lamb = 0.5 and temperature = 0.5 (attributes of the model), hard labels
    for case, tct, lamb, temp, w in (("dhr_tct", True, 1.0, 1.0, D), ("dhr_tct_half", True, 0.5, 0.5, D), ("dhr_hard", False, 1.0, 1.0, H)):
        lex, sem, tea = leaf(grid((R, C), 40)), leaf(grid((R, C), 24)), torch.from_numpy(grid((R, C), 48))
        s = stub(DM.DHRModel, R, n, tct, tea, (lex, sem), (eye, eye), lamb, temp, dlr_out_dim=None)
        o = DM.DHRModel.forward(s, {"input_ids": 1}, {"input_ids": 1})
        assert torch.equal(o.scores, lex.detach() + lamb * sem.detach())
        keep(f"{case}_{tag}", R, n, lex, sem, tea if tct else None, lamb, temp, w, SPLIT, o.loss, o.scores)
    # the Aggretriever model's forward: --tct, hard labels with semantic reps, hard labels without
    remove = cal_remove_dim(C)
    assert 0 <= remove
    front = lambda rows: torch.zeros(rows, remove)  # noqa: E731
    for case, tct, with_sem, w in (("agg_tct", True, True, D), ("agg_hard_sem", False, True, D), ("agg_hard_nosem", False, False, H)):
        lex, sem, tea = leaf(grid((R, C), 40)), leaf(grid((R, C), 24)) if with_sem else None, torch.from_numpy(grid((R, C), 48))
        q_reps = (torch.cat([front(R), lex], 1), sem)
        p_reps = (torch.cat([front(C), eye], 1), eye if with_sem else None)
        s = stub(AM.DenseModel, R, n, tct, tea, q_reps, p_reps, 1.0, 1.0, skip_mlm=False, agg_dim=C, semi_aggregate=True)
        o = AM.DenseModel.forward(s, {"input_ids": 1}, {"input_ids": 1})
        assert torch.equal(o.scores, lex.detach() + (sem.detach() if with_sem else 0))
        keep(f"{case}_{tag}", R, n, lex, sem, tea if tct else None, 1.0, 1.0, w, SPLIT, o.loss, o.scores)
    # Dense/modeling.py:134-140 (ColBERT/modeling.py:154-160 is the same call)
    lex = leaf(grid((R, C), 40))
    target = torch.arange(R, dtype=torch.long) * n
    keep(f"dense_ce_{tag}", R, n, lex, None, None, 1.0, 1.0, H, SPLIT, nn.CrossEntropyLoss(reduction="mean")(lex, target), lex)
    # ColBERT/modeling.py:146-150: the teacher's [R, n] scores padded with -20 into the listwise layout, temperature 1
    lex, t_small = leaf(grid((R, C), 40)), torch.from_numpy(grid((R, n), 48))
    tea = torch.nn.functional.pad(input=t_small * 1.0, pad=(0, C), mode="constant", value=-20)
    tea = tea.view(-1)[:-C].view(R, -1)
    assert tuple(tea.shape) == (R, C)
    loss = nn.KLDivLoss(reduction="batchmean")(nn.functional.log_softmax(lex, dim=-1), nn.Softmax(dim=-1)(tea))
    keep(f"colbert_kd_{tag}", R, n, lex, None, tea.contiguous(), 1.0, 1.0, H, (1.0, 1.0, 1.0), loss, lex)

out["names"] = np.array(names)
path = os.path.join(HERE, "train_loss_golden.npz")
np.savez_compressed(path, **out)
assert os.path.getsize(path) < 256 * 1024
print(os.path.getsize(path), "bytes;", len(names), "cases")
for k in names:
    print(k, float(out[k + "_loss"]))
