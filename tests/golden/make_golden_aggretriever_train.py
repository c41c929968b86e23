#!/usr/bin/env python
"""Golden vectors for the Aggretriever training ops (dhr_amd/aggretriever_train.py): runs the REFERENCE's own code with autograd on, on the CPU.

No-MLM chain: DenseModel.encode_passage(stub, psg, True), called unbound on a stub `self` whose language model returns seeded hidden states,
with psg a transformers.BatchEncoding (the method reads psg.input_ids); a forward hook on the stub's term_weight_trans retains the gradient of
the term weights.  Then the reference's aggregate and .backward(G) with a seeded G [B, dims] of mixed signs and zeros, once per aggregation.
A case is redrawn until its designed repeats hold and no weight is exactly 0.  Aggregate alone: a dense leaf [B, V] of quantised values
(steps of 0.25, mixed signs) with designed ties.  Stored: inputs, reps, aggregated output, G, d reps and dw.
Run where the reference checkout is at hand (it is not part of the repository):
    python tests/golden/make_golden_aggretriever_train.py <reference checkout>"""
import os
import sys
import types

import numpy as np
import torch
from transformers import BatchEncoding

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, sys.argv[1])
from tevatron.Aggretriever import modeling as AM  # noqa: E402
from tevatron.Aggretriever.utils import aggregate  # noqa: E402

torch.manual_seed(20261018)
rng = np.random.default_rng(20261018)
out = {}
V = 30522
AGGS = [(640, True), (768, True), (128, True), (640, False), (768, False)]


def quantised(shape, scale=2.0, step=0.25, clip=7.75):
    return np.clip(np.round(rng.standard_normal(shape) * scale / step) * step, -clip, clip)


def key(dims, full):
    return "{}{}".format(dims, "f" if full else "s")


def run_aggs(name, reps, aggs, retain):
    """reps: a tensor with a graph behind it; for each aggregation: output, G, d reps (and whatever `retain` holds, through the callback)"""
    for dims, full in aggs:
        leaf = reps.detach().clone().requires_grad_(True)
        agg = aggregate(leaf, dims, full=full)
        G = quantised((reps.shape[0], dims), 1.0, 0.25).astype(np.float32)        # mixed signs, about a tenth of the entries zero
        assert (G == 0).any() and (G < 0).any() and (G > 0).any()
        agg.backward(torch.from_numpy(G))
        k = name + "_" + key(dims, full)
        out[k + "_out"] = agg.detach().numpy()
        out[k + "_G"] = G
        out[k + "_dreps"] = leaf.grad.numpy()
        retain(k, leaf.grad)


def chain(name, ids, H, bias, ok):
    B, L = ids.shape
    for attempt in range(5000):
        hidden = torch.from_numpy(rng.standard_normal((B, L, H)).astype(np.float16).astype(np.float32))
        lin = torch.nn.Linear(H, 1)
        if bias is not None:
            with torch.no_grad():
                lin.bias.fill_(bias)
        stub = types.SimpleNamespace(lm_p=lambda **kw: types.SimpleNamespace(hidden_states=[hidden]), term_weight_trans=lin, pooler=None)
        kept = []

        def keep(mod, inp, res):
            res.retain_grad()
            kept.append(res)

        lin.register_forward_hook(keep)
        psg = BatchEncoding({"input_ids": torch.from_numpy(ids), "attention_mask": torch.ones((B, L), dtype=torch.long)})
        reps, semantic = AM.DenseModel.encode_passage(stub, psg, True)
        w = kept[0].detach()[..., 0].numpy()
        if (w == 0).any() or not ok(w):
            continue
        assert semantic is None and tuple(reps.shape) == (B, V)
        out[name + "_ids"] = ids                                                  # [B, L] int64
        out[name + "_w"] = w                                                      # [B, L-1] fp32
        out[name + "_reps"] = reps.detach().numpy()

        def through_head(k, dreps):
            kept[0].grad = None
            reps.backward(dreps, retain_graph=True)
            out[k + "_dw"] = kept[0].grad[..., 0].numpy().copy()                  # [B, L-1]

        run_aggs(name, reps, AGGS, through_head)
        return
    raise RuntimeError(name + ": no draw with the designed repeats")


# the no-MLM chain: B = 3, L = 9 (token 0 takes no part)
ids = np.array([[101, 2000, 2000, 3000, 5, 441, 7000, 102, 0],          # a repeat (t = 0, 1), ids inside the removed leading columns, one trailing pad
                [101, 4000, 30521, 9000, 4000, 442, 102, 0, 0],         # a repeat (t = 0, 3), the last vocabulary id, the first kept id of 640 / semi
                [101, 1080 + 23 * 1280, 29440, 102, 0, 0, 0, 0, 0]],    # the last real pair of 640 / full's last group and its first column; pads repeat id 0
               np.int64)
chain("chain", ids, 16, None, lambda w: 0 < w[0, 0] < w[0, 1] and w[1, 0] > w[1, 3] > 0 and (w[:, :3] > 0).all() and (w[2, 3:] > 0).sum() >= 2)
# every weight negative (Linear bias -6): the zero wins everywhere
chain("neg", ids, 16, -6.0, lambda w: (w < 0).all())


def alone(name, x, aggs):
    out[name + "_x4"] = np.round(x * 4).astype(np.int8)                             # the leaf, times 4
    run_aggs(name, torch.from_numpy(x.astype(np.float32)), aggs, lambda k, g: None)


# aggregate alone at the production vocabulary: designed ties for (640, full): groups of 1280 columns, 24 groups, the last one padded from column 1082
x = quantised((2, V))
x[0, 3 * 1280 + 10] = x[0, 7 * 1280 + 10] = 9.0                                      # an equal maximum in two groups: the first
x[0, 5 * 1280 + 40] = x[0, 2 * 1280 + 41] = 9.5                                      # pos == neg, non-zero: the negative branch
for c in (1100, 1101):                                                              # real entries all negative: the zero padding wins both columns
    x[0, np.arange(23) * 1280 + c] = -np.abs(x[0, np.arange(23) * 1280 + c]) - 0.25
x[1, np.arange(23) * 1280 + 1200] = -1.0                                             # pos in the padding (0), neg positive
alone("dense", x, AGGS)
# small vocabularies the reference's geometry accepts
for B in (1, 5):
    alone("v186b%d" % B, quantised((B, 186)), [(16, True)])                          # remove 26, 5 groups of 32
    alone("v57b%d" % B, quantised((B, 57)), [(9, False)])                            # remove 3 (odd), 6 groups of 9, odd V

path = os.path.join(HERE, "aggretriever_train_golden.npz")
np.savez_compressed(path, **out)
print(os.path.getsize(path), "bytes;", {k: getattr(v, "shape", None) for k, v in out.items()})
