#!/usr/bin/env python
"""Golden vectors for the lexical head with the vocabulary projection fused in (dhr_amd/lexical_proj.py): runs the REFERENCE's own code --
DHRModel.encode_passage / encode_query and the Aggretriever DenseModel.encode_passage(skip_mlm=False), called unbound on a stub `self`, then
densify, aggregate (full and semi) and merge_reps -- and stores inputs + outputs.  The stub's language model returns
logits = F.linear(hidden, W, b) in fp32 on the CPU from seeded EXACT-ARITHMETIC operands

    hidden = randint(-8..8) / 4,   W = choice(-1, 0, 0, 1) / 8,   b = randint(-16..16) / 32

so every partial sum of a logit is a multiple of 2^-5 below 2^9: fp32 accumulation is exact in any order and the logits are fp16 values.
The library is given hidden, W and b; the logits themselves are not stored.
Run where a checkout of the reference is at hand (it is not part of the repository):
    python tests/golden/make_golden_lexical_proj.py <path to the reference checkout>"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, sys.argv[1])
from tevatron.Aggretriever import modeling as AM  # noqa: E402
from tevatron.Aggretriever import utils as AU  # noqa: E402
from tevatron.DHR import modeling as DM  # noqa: E402
from tevatron.DHR import utils as DU  # noqa: E402

torch.manual_seed(20261018)
rng = np.random.default_rng(20261018)
out = {}


def exact_operands(B, L, V, H):
    hidden = rng.integers(-8, 9, (B, L, H)).astype(np.float32) / 4
    W = rng.choice(np.array([-1, 0, 0, 1], np.float32), (V, H)) / 8
    b = rng.integers(-16, 17, V).astype(np.float32) / 32
    return hidden, W, b


def stub(enc, hidden, W, b, H_enc, bias=None):
    """lm: last hidden state `enc` (term weights, [CLS]) and the MLM logits as the vocabulary projector makes them from `hidden`."""
    logits = torch.nn.functional.linear(torch.from_numpy(hidden), torch.from_numpy(W), torch.from_numpy(b))
    lm = lambda **kw: types.SimpleNamespace(hidden_states=[enc], logits=logits)  # noqa: E731
    lin = torch.nn.Linear(H_enc, 1)
    if bias is not None:
        with torch.no_grad():
            lin.bias.fill_(bias)
    return types.SimpleNamespace(lm_p=lm, lm_q=lm, term_weight_trans=lin, softmax=torch.nn.Softmax(dim=-1), pooler=None), logits


def near_midpoint(x):
    """entries whose fp16 rounding flips within the tests' tolerance (1e-5 |x| + 1e-30): the goldens must have none."""
    x = np.asarray(x, np.float64)
    t = 1e-5 * np.abs(x) + 1e-30
    return int(((x - t).astype(np.float16) != (x + t).astype(np.float16)).sum())


def case(name, *args, **kw):
    for attempt in range(50):
        keep = dict(out)
        _case(name, *args, **kw)
        keys = [k for k in (name + "_dval", name + "_cls", name + "_afull", name + "_asemi") if k in out]
        if sum(near_midpoint(out[k]) for k in keys) == 0:
            return
        out.clear()
        out.update(keep)                                   # (the next draw of the term-weight Linear and of the encoder states)
    raise RuntimeError(name + ": no draw without fp16 midpoints")


def _case(name, hidden, W, b, dims, remove, agg_dim, mask, bias=None, query=False, H_enc=8):
    B, L, _ = hidden.shape
    enc = torch.from_numpy(rng.standard_normal((B, L, H_enc)).astype(np.float16).astype(np.float32))
    s, logits = stub(enc, hidden, W, b, H_enc, bias)
    # the recipe's promise: the fp32 logits are the exact ones and are fp16 values
    exact = hidden.astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64)
    assert np.array_equal(logits.numpy().astype(np.float64), exact) and np.array_equal(exact.astype(np.float16).astype(np.float64), exact)
    batch = {"input_ids": torch.zeros((B, L), dtype=torch.long), "attention_mask": torch.from_numpy(mask)}
    with torch.no_grad():
        reps, cls = (DM.DHRModel.encode_query if query else DM.DHRModel.encode_passage)(s, batch)
        agg_reps, _ = AM.DenseModel.encode_passage(s, batch, False)
        w = s.term_weight_trans(enc[:, 1:])[..., 0]
    assert torch.equal(reps, agg_reps)
    out[name + "_hidden"] = hidden.astype(np.float16)                       # [B, L, H]: the library reads the [:, 1:] view
    out[name + "_W"] = W.astype(np.float16)                                 # [V, H]
    out[name + "_bias"] = b                                                 # [V] fp32 (fp16 values)
    out[name + "_w"] = w.numpy().astype(np.float32)                         # [B, L-1]
    out[name + "_mask"] = mask                                              # [B, L]
    out[name + "_reps"] = reps.numpy()
    out[name + "_cls"] = cls.numpy()
    out[name + "_geom"] = np.array([dims, remove, agg_dim])
    if dims:
        v, i = DU.densify(reps, dims, remove_dims=remove)
        rec_v = np.zeros((B, dims + H_enc), np.float16)                     # encode.py:155-170 / 179-194
        rec_v[:, :dims] = v.numpy()
        rec_v[:, dims:] = cls.numpy()
        out[name + "_dval"], out[name + "_didx"] = v.numpy(), i.numpy()
        out[name + "_drec_v"], out[name + "_drec_i"] = rec_v, i.numpy().astype(np.uint8)
    for full in (True, False):
        tag = "_afull" if full else "_asemi"
        a = AU.aggregate(reps, agg_dim, full=full)
        merged = AM.DenseModel.merge_reps(a, cls)                           # Aggretriever/modeling.py:328-334
        out[name + tag] = a.numpy()
        out[name + tag + "_rec"] = merged.numpy().astype(np.float16)        # encode.py:149-153 / 174-178


# production vocabulary: BERT 30522, densify 768 / 570, aggregate 640; H = 16 keeps the file small
B, L, V, H = 2, 4, 30522, 16
hidden, W, b = exact_operands(B, L, V, H)
W[570 + 5] = W[570 + 768 + 5] = np.sign(hidden[0, 2]) / 8                   # a group tie: two columns with identical, large logits
b[570 + 5] = b[570 + 768 + 5] = 0.5
mask = np.array([[1, 1, 1, 1], [1, 1, 1, 0]], np.int64)
case("prod", hidden, W, b, 768, 570, 640, mask)

# small vocabulary (cal_remove_dim still uses 30522: agg 8 -> full remove 10, groups of 16; semi remove 2, groups of 8)
B, L, V, H = 5, 7, 202, 24
hidden, W, b = exact_operands(B, L, V, H)
W[2 + 3] = W[2 + 8 + 3] = np.sign(hidden[0, 3]) / 8                         # group tie: the first group wins
b[2 + 3] = b[2 + 8 + 3] = 0.25
hidden[1, 4] = hidden[1, 2]                                                 # token tie: identical logits
mask = np.ones((B, L), np.int64)
mask[0, 5:] = 0                                                             # padding
mask[1, 3] = 0                                                              # a masked token between unmasked ones
mask[3, 1:] = 0                                                             # fully masked passage (the CLS position is not part of the head)
mask[4, 3:] = 0                                                             # masked from the middle
case("small", hidden, W, b, 8, 2, 8, mask)

# negative term weights everywhere (LinearPooler has no ReLU), padding, a fully masked row, queries; H = 8 * 9
B, L, V, H = 3, 6, 762, 72
hidden, W, b = exact_operands(B, L, V, H)
mask = np.ones((B, L), np.int64)
mask[1, 3:] = 0
mask[2, 1:] = 0
case("neg", hidden, W, b, 64, 58, 8, mask, bias=-6.0, query=True)

# aggregate with a negative remove on a small vocabulary (agg 700: full remove -278 pads 278 zeros to one group of 1400; semi remove 422)
B, L, V, H = 3, 5, 1122, 24
hidden, W, b = exact_operands(B, L, V, H)
mask = np.ones((B, L), np.int64)
mask[2, 2:] = 0
case("pad", hidden, W, b, 0, 0, 700, mask, bias=-0.5)

path = os.path.join(HERE, "lexical_proj_golden.npz")
np.savez_compressed(path, **out)
print(os.path.getsize(path), "bytes;", {k: getattr(v, "shape", None) for k, v in out.items()})
