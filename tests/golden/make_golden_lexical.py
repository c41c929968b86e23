#!/usr/bin/env python
"""Golden vectors for the fused lexical head (dhr_amd/lexical.py): runs the REFERENCE's own code -- DHRModel.encode_passage /
encode_query and the Aggretriever DenseModel.encode_passage(skip_mlm=False), called unbound on a stub `self` whose language model returns
seeded hidden states and logits, then densify, aggregate (full and semi) and merge_reps -- and stores inputs + outputs.  The logits are
fp32 tensors holding fp16-representable values (what autocast hands the reference's softmax); the library is given them as fp16.
Run in the build container only (the reference checkout is not part of the repository):  python tests/golden/make_golden_lexical.py"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
from tevatron.Aggretriever import modeling as AM  # noqa: E402
from tevatron.Aggretriever import utils as AU  # noqa: E402
from tevatron.DHR import modeling as DM  # noqa: E402
from tevatron.DHR import utils as DU  # noqa: E402

torch.manual_seed(20261016)
rng = np.random.default_rng(20261016)
out = {}


def stub(hidden, logits, H, bias=None):
    lm = lambda **kw: types.SimpleNamespace(hidden_states=[hidden], logits=logits)  # noqa: E731
    lin = torch.nn.Linear(H, 1)
    if bias is not None:
        with torch.no_grad():
            lin.bias.fill_(bias)
    return types.SimpleNamespace(lm_p=lm, lm_q=lm, term_weight_trans=lin, softmax=torch.nn.Softmax(dim=-1), pooler=None)


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
        out.update(keep)
        # (the next draw of the term-weight Linear -- and of the hidden states where the case does not fix them -- keeps the designed ties)
    raise RuntimeError(name + ": no draw without fp16 midpoints")


def _case(name, B, L, V, H, dims, remove, agg_dim, mask, logits, hidden=None, bias=None, query=False):
    hidden = torch.from_numpy(rng.standard_normal((B, L, H)).astype(np.float16).astype(np.float32)) if hidden is None else hidden
    lg = torch.from_numpy(logits.astype(np.float16).astype(np.float32))
    s = stub(hidden, lg, H, bias)
    batch = {"input_ids": torch.zeros((B, L), dtype=torch.long), "attention_mask": torch.from_numpy(mask)}
    with torch.no_grad():
        reps, cls = (DM.DHRModel.encode_query if query else DM.DHRModel.encode_passage)(s, batch)
        agg_reps, _ = AM.DenseModel.encode_passage(s, batch, False)
        w = s.term_weight_trans(hidden[:, 1:])[..., 0]
    assert torch.equal(reps, agg_reps)
    out[name + "_logits"] = logits.astype(np.float16)                       # [B, L, V]: the library reads the [:, 1:] view
    out[name + "_w"] = w.numpy().astype(np.float32)                         # [B, L-1]
    out[name + "_mask"] = mask                                              # [B, L]
    out[name + "_reps"] = reps.numpy()
    out[name + "_cls"] = cls.numpy()
    if dims:
        v, i = DU.densify(reps, dims, remove_dims=remove)
        rec_v = np.zeros((B, dims + H), np.float16)                         # encode.py:155-170 / 179-194
        rec_i = np.zeros((B, dims), np.uint8)
        rec_v[:, :dims] = v.numpy()
        rec_i[:, :dims] = i.numpy().astype(np.uint8)
        rec_v[:, dims:] = cls.numpy()
        out[name + "_dval"], out[name + "_didx"] = v.numpy(), i.numpy()
        out[name + "_drec_v"], out[name + "_drec_i"] = rec_v, rec_i
        out[name + "_geom"] = np.array([dims, remove, agg_dim])
    for full in (True, False):
        if not agg_dim:
            continue
        tag = "_afull" if full else "_asemi"
        a = AU.aggregate(reps, agg_dim, full=full)
        merged = AM.DenseModel.merge_reps(a, cls)                           # Aggretriever/modeling.py:328-334
        out[name + tag] = a.numpy()
        out[name + tag + "_rec"] = merged.numpy().astype(np.float16)        # encode.py:149-153 / 174-178


def quantised(shape, scale=2.0, step=0.25):
    return np.round(rng.standard_normal(shape) * scale / step) * step


# production vocabulary: BERT 30522, densify 768 / 570, aggregate 640 (full: remove -198, 24 groups of 1280; semi: remove 442, 47 groups)
B, L, V, H = 2, 4, 30522, 16
lg = quantised((B, L, V))
lg[0, 2, 570 + 5] = lg[0, 2, 570 + 768 + 5] = 9.0                           # equal maxima in two groups of one slice
mask = np.array([[1, 1, 1, 1], [1, 1, 1, 0]], np.int64)
case("prod", B, L, V, H, 768, 570, 640, mask, lg)

# small vocabularies (cal_remove_dim still uses 30522: agg 8 -> full remove 10, groups of 16; semi remove 2, groups of 8)
B, L, V, H = 5, 7, 202, 8
lg = quantised((B, L, V))
lg[0, 3, 2 + 3] = lg[0, 3, 2 + 8 + 3] = 12.0                               # group tie: the first group wins
lg[1, 2] = lg[1, 4]                                                         # token tie: identical logits and hidden states
lg[1, :, 40:60] = -np.inf                                                   # -inf logits: p = 0, contributions are zeros signed like w
lg[2, 5, :150] = -np.inf
hidden = torch.from_numpy(rng.standard_normal((B, L, H)).astype(np.float16).astype(np.float32))   # fp16 values, like the CLS reps under autocast
hidden[1, 4] = hidden[1, 2]
mask = np.ones((B, L), np.int64)
mask[0, 5:] = 0                                                             # padding
mask[3, 1:] = 0                                                             # fully masked row (the CLS position is not part of the head)
mask[4, 3:] = 0
case("small", B, L, V, H, 8, 2, 8, mask, lg, hidden=hidden)

# negative term weights everywhere (LinearPooler has no ReLU), padding, queries
B, L, V, H = 3, 6, 202, 8
lg = quantised((B, L, V))
mask = np.ones((B, L), np.int64)
mask[1, 3:] = 0
mask[2, 1:] = 0
case("neg", B, L, V, H, 8, 2, 8, mask, lg, bias=-6.0, query=True)

# aggregate with a negative remove on a small vocabulary (agg 700: full remove -278 pads 278 zeros to one group of 1400; semi remove 422)
B, L, V, H = 3, 5, 1122, 8
lg = quantised((B, L, V))
mask = np.ones((B, L), np.int64)
mask[2, 2:] = 0
case("pad", B, L, V, H, 0, 0, 700, mask, lg, bias=-0.5)

# error texts: densify (ValueError) and the reference aggregate's view (RuntimeError)
errs = []
for fn in (lambda: DU.densify(torch.zeros(2, 30), 7, remove_dims=1),
           lambda: AU.aggregate(torch.zeros(2, 1000), 640, full=True),
           lambda: AU.aggregate(torch.zeros(2, 1000), 8, full=True),
           lambda: AU.aggregate(torch.zeros(2, 1000), 8, full=False),
           lambda: AU.aggregate(torch.zeros(2, 5), 8, full=False)):
    try:
        fn()
        errs.append("")
    except (ValueError, RuntimeError) as e:
        errs.append(type(e).__name__ + ": " + str(e))
out["errors"] = np.array(errs)
np.savez_compressed(os.path.join(HERE, "lexical_golden.npz"), **out)
print(os.path.getsize(os.path.join(HERE, "lexical_golden.npz")), "bytes;", {k: getattr(v, "shape", None) for k, v in out.items()})
print(errs)
