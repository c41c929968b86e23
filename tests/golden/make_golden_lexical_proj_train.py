#!/usr/bin/env python
"""Golden vectors for the differentiable lexical head with the vocabulary projection fused in (dhr_amd/lexical_proj_train.py): runs the
REFERENCE's own code -- DHRModel.encode_passage / encode_query, called unbound on a stub `self` -- with autograd on.  The stub's language
model returns logits = F.linear(hidden, W, b) in fp32 on the CPU, with hidden, W and b leaves that require grad, from the seeded
EXACT-ARITHMETIC operands of make_golden_lexical_proj.py

    hidden = randint(-8..8) / 4,   W = choice(-1, 0, 0, 1) / 8,   b = randint(-16..16) / 32

(every partial sum of a logit is a multiple of 2^-5 below 2^9: fp32 accumulation is exact in any order and the logits are fp16 values).  A
forward hook on the stub's term_weight_trans retains the gradient of the term weights, and sum(G * reps) is backpropagated with a seeded
upstream G [B, V] of mixed signs and zeros.  Stored: inputs, reps, G, dhidden [B, L, H] (row 0 zero), dbias, the term weights' gradient and
dW (for the production vocabulary a seeded sample of 2304 rows that holds rows 0, 255, 256 and the last 64).  A case is redrawn until no
(b, v) entry is a near-tie (two token contributions within 1e-5 * |max| + 1e-30 of each other without being equal).
Run where a checkout of the reference is at hand (it is not part of the repository):
    python tests/golden/make_golden_lexical_proj_train.py <path to the reference checkout>"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, sys.argv[1])
from tevatron.DHR import modeling as DM  # noqa: E402

torch.manual_seed(20261019)
rng = np.random.default_rng(20261019)
out = {}


def exact_operands(B, L, V, H):
    hidden = rng.integers(-8, 9, (B, L, H)).astype(np.float32) / 4
    W = rng.choice(np.array([-1, 0, 0, 1], np.float32), (V, H)) / 8
    b = rng.integers(-16, 17, V).astype(np.float32) / 32
    return hidden, W, b


def near_ties(x, w, mask):
    """(b, v) entries with a token contribution within the tests' tolerance of the maximum without being equal to it (float64)"""
    e = np.exp(x - x.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    c = (p * w.astype(np.float64)[..., None]) * mask[:, 1:].astype(np.float64)[..., None]
    top = c.max(1, keepdims=True)
    return int((((top - c) <= 1e-5 * np.abs(top) + 1e-30) & (c != top)).any(1).sum())


def case(name, hidden, W, b, mask, bias=None, query=False, same_enc=None, H_enc=8, sample=None):
    B, L, H = hidden.shape
    V = W.shape[0]
    exact = hidden.astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64)
    for attempt in range(50):
        enc = torch.from_numpy(rng.standard_normal((B, L, H_enc)).astype(np.float16).astype(np.float32))
        if same_enc is not None:                                                   # identical encoder states: identical term weights
            enc[same_enc[0], same_enc[1]] = enc[same_enc[0], same_enc[2]]
        th, tW, tb = (torch.from_numpy(a.copy()).requires_grad_(True) for a in (hidden, W, b))
        logits = torch.nn.functional.linear(th, tW, tb)
        # the recipe's promise: the fp32 logits are the exact ones and are fp16 values
        assert np.array_equal(logits.detach().numpy().astype(np.float64), exact) and np.array_equal(exact.astype(np.float16).astype(np.float64), exact)
        lm = lambda **kw: types.SimpleNamespace(hidden_states=[enc], logits=logits)  # noqa: E731
        lin = torch.nn.Linear(H_enc, 1)
        if bias is not None:
            with torch.no_grad():
                lin.bias.fill_(bias)
        s = types.SimpleNamespace(lm_p=lm, lm_q=lm, term_weight_trans=lin, softmax=torch.nn.Softmax(dim=-1), pooler=None)
        kept = []

        def keep(mod, inp, res):
            res.retain_grad()
            kept.append(res)

        lin.register_forward_hook(keep)
        batch = {"input_ids": torch.zeros((B, L), dtype=torch.long), "attention_mask": torch.from_numpy(mask)}
        reps, _ = (DM.DHRModel.encode_query if query else DM.DHRModel.encode_passage)(s, batch)
        G = (np.round(rng.standard_normal((B, V)) / 0.25) * 0.25).astype(np.float32)  # mixed signs, about a tenth of the entries zero
        (torch.from_numpy(G) * reps).sum().backward()
        w = kept[0].detach()[..., 0].numpy().astype(np.float32)
        if near_ties(exact[:, 1:], w, mask):
            continue                                                               # (the next draw of the Linear and of the encoder states)
        out[name + "_hidden"] = hidden.astype(np.float16)                          # [B, L, H]
        out[name + "_W"] = W.astype(np.float16)                                    # [V, H]
        out[name + "_bias"] = b                                                    # [V] fp32 (fp16 values)
        out[name + "_w"] = w                                                       # [B, L-1]
        out[name + "_mask"] = mask                                                 # [B, L]
        out[name + "_reps"] = reps.detach().numpy()
        out[name + "_G"] = G
        out[name + "_dhidden"] = th.grad.numpy()                                   # [B, L, H]
        out[name + "_dbias"] = tb.grad.numpy()                                     # [V]
        out[name + "_dw"] = kept[0].grad[..., 0].numpy()                           # [B, L-1]
        rows = np.arange(V) if sample is None else sample
        out[name + "_dW_rows"] = rows.astype(np.int32)
        out[name + "_dW"] = tW.grad.numpy()[rows]                                  # [rows, H]
        assert not out[name + "_dhidden"][:, 0].any() and (G == 0).any() and (G < 0).any() and (G > 0).any()
        return
    raise RuntimeError(name + ": no draw without near-ties")


# production vocabulary: BERT 30522; H = 16 keeps the file small
B, L, V, H = 2, 4, 30522, 16
hidden, W, b = exact_operands(B, L, V, H)
mask = np.array([[1, 1, 1, 1], [1, 1, 1, 0]], np.int64)
fixed = np.concatenate([[0, 255, 256], np.arange(V - 64, V)])
rest = np.setdiff1d(np.arange(V), fixed)
sample = np.sort(np.concatenate([fixed, rng.choice(rest, 2304 - len(fixed), replace=False)]))
case("prod", hidden, W, b, mask, sample=sample)

# a fully masked passage, one masked from the middle, a masked token between live ones, a token tie
B, L, V, H = 5, 7, 202, 24
hidden, W, b = exact_operands(B, L, V, H)
hidden[1, 4] = hidden[1, 2]                                                        # token tie: identical logits and term weights
mask = np.ones((B, L), np.int64)
mask[0, 5:] = 0                                                                    # padding
mask[1, 3] = 0                                                                     # a masked token between unmasked ones
mask[3, 1:] = 0                                                                    # fully masked passage (the CLS position is not part of the head)
mask[4, 3:] = 0                                                                    # masked from the middle
case("small", hidden, W, b, mask, same_enc=(1, 4, 2))

# negative term weights everywhere (LinearPooler has no ReLU), padding, a fully masked row, queries; H = 8 * 9
B, L, V, H = 3, 6, 762, 72
hidden, W, b = exact_operands(B, L, V, H)
mask = np.ones((B, L), np.int64)
mask[1, 3:] = 0
mask[2, 1:] = 0
case("neg", hidden, W, b, mask, bias=-6.0, query=True)

path = os.path.join(HERE, "lexical_proj_train_golden.npz")
np.savez_compressed(path, **out)
print(os.path.getsize(path), "bytes;", {k: getattr(v, "shape", None) for k, v in out.items()})
