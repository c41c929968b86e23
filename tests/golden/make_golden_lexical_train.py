#!/usr/bin/env python
"""Golden vectors for the differentiable lexical head (dhr_amd/lexical_train.py): runs the REFERENCE's own code -- DHRModel.encode_passage /
encode_query, called unbound on a stub `self` whose language model returns seeded hidden states and logits -- with autograd on.  The logits
are a leaf [B, L, V] (fp32 holding fp16-representable values, what autocast hands the reference's softmax), a forward hook on the stub's
term_weight_trans retains the gradient of the term weights, and reps.backward(G) runs with a seeded upstream G [B, V] of mixed signs and
zeros.  Stored: inputs, reps, G, dL/dlogits ([B, L, V], row 0 zero) and dL/dw.  A case is redrawn until no (b, v) entry is a near-tie
(two token contributions within 1e-5 * |max| + 1e-30 of each other without being equal), so the tests need no exemption on the goldens.
Run in the build container only (the reference checkout is not part of the repository):  python tests/golden/make_golden_lexical_train.py"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
from tevatron.DHR import modeling as DM  # noqa: E402

torch.manual_seed(20261017)
rng = np.random.default_rng(20261017)
out = {}


def stub(hidden, logits, H, bias=None):
    lm = lambda **kw: types.SimpleNamespace(hidden_states=[hidden], logits=logits)  # noqa: E731
    lin = torch.nn.Linear(H, 1)
    if bias is not None:
        with torch.no_grad():
            lin.bias.fill_(bias)
    return types.SimpleNamespace(lm_p=lm, lm_q=lm, term_weight_trans=lin, softmax=torch.nn.Softmax(dim=-1), pooler=None)


def near_ties(logits, w, mask):
    """(b, v) entries with a token contribution within the tests' tolerance of the maximum without being equal to it (float64)"""
    x = logits[:, 1:].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(x - x.max(-1, keepdims=True))
        p = e / e.sum(-1, keepdims=True)
    c = (p * w.astype(np.float64)[..., None]) * mask[:, 1:].astype(np.float64)[..., None]
    top = c.max(1, keepdims=True)
    return int((((top - c) <= 1e-5 * np.abs(top) + 1e-30) & (c != top)).any(1).sum())


def quantised(shape, scale=2.0, step=0.25):
    return np.round(rng.standard_normal(shape) * scale / step) * step


def case(name, B, L, V, H, mask, logits, hidden=None, bias=None, query=False):
    for attempt in range(50):
        hid = torch.from_numpy(rng.standard_normal((B, L, H)).astype(np.float16).astype(np.float32)) if hidden is None else hidden
        lg = torch.from_numpy(logits.astype(np.float16).astype(np.float32)).requires_grad_(True)
        s = stub(hid, lg, H, bias)
        kept = []

        def keep(mod, inp, res):
            res.retain_grad()
            kept.append(res)

        s.term_weight_trans.register_forward_hook(keep)
        batch = {"input_ids": torch.zeros((B, L), dtype=torch.long), "attention_mask": torch.from_numpy(mask)}
        reps, _ = (DM.DHRModel.encode_query if query else DM.DHRModel.encode_passage)(s, batch)
        G = quantised((B, V), 1.0, 0.25).astype(np.float32)                        # mixed signs, about a tenth of the entries zero
        reps.backward(torch.from_numpy(G))
        w = kept[0].detach()[..., 0].numpy().astype(np.float32)
        if near_ties(logits.astype(np.float16).astype(np.float32), w, mask):
            continue                                                              # (the next draw of the Linear keeps the designed ties)
        out[name + "_logits"] = logits.astype(np.float16)                          # [B, L, V]
        out[name + "_w"] = w                                                       # [B, L-1]
        out[name + "_mask"] = mask                                                 # [B, L]
        out[name + "_reps"] = reps.detach().numpy()
        out[name + "_G"] = G
        out[name + "_dlogits"] = lg.grad.numpy()                                   # [B, L, V]
        out[name + "_dw"] = kept[0].grad[..., 0].numpy()                           # [B, L-1]
        assert not out[name + "_dlogits"][:, 0].any() and (G == 0).any() and (G < 0).any() and (G > 0).any()
        return
    raise RuntimeError(name + ": no draw without near-ties")


# production vocabulary (BERT 30522), one passage, the last token padding
B, L, V, H = 1, 4, 30522, 16
case("prod", B, L, V, H, np.array([[1, 1, 1, 0]], np.int64), quantised((B, L, V)))

# the "small" design of the encoding goldens: an exact token tie (identical logits and hidden states), -inf logits, padding, a fully masked row
B, L, V, H = 5, 7, 202, 8
lg = quantised((B, L, V))
lg[1, 2] = lg[1, 4]
lg[1, :, 40:60] = -np.inf
lg[2, 5, :150] = -np.inf
hidden = torch.from_numpy(rng.standard_normal((B, L, H)).astype(np.float16).astype(np.float32))
hidden[1, 4] = hidden[1, 2]
mask = np.ones((B, L), np.int64)
mask[0, 5:] = 0
mask[3, 1:] = 0
mask[4, 3:] = 0
case("small", B, L, V, H, mask, lg, hidden=hidden)

# negative term weights everywhere (LinearPooler has no ReLU), padding, queries
B, L, V, H = 3, 6, 202, 8
mask = np.ones((B, L), np.int64)
mask[1, 3:] = 0
mask[2, 1:] = 0
case("neg", B, L, V, H, mask, quantised((B, L, V)), bias=-6.0, query=True)

path = os.path.join(HERE, "lexical_train_golden.npz")
np.savez_compressed(path, **out)
print(os.path.getsize(path), "bytes;", {k: getattr(v, "shape", None) for k, v in out.items()})
