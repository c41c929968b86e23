"""The loss of a training step, fused with its gradient, on the HIP op `dhr_train_loss`.

The reference ends a step on an eager tail (tevatron/DHR/modeling.py:170-197, Aggretriever/modeling.py:184-213, ColBERT/modeling.py:146-160,
Dense/modeling.py:134-140): one fusion, three log_softmax, three scaled softmax of the teacher scores, three KLDivLoss(batchmean) and the
weighted sum -- some twenty small launches forward and more backward on [effective_bsz, effective_bsz * train_n_passages] matrices, with a
dozen temporaries of that shape kept for autograd.  Here

    hybrid_loss(lexical_scores, semantic_scores=None, teacher_scores=None, *, train_n_passages, lamb, temperature, weights, teacher_split)
    dhr_loss(lexical_scores, semantic_scores, teacher_scores=None, *, train_n_passages, lamb, temperature)       DHR/modeling.py:170-197
    aggretriever_loss(lexical_scores, semantic_scores=None, teacher_scores=None, *, train_n_passages, temperature)   Aggretriever/modeling.py:184-213
    contrastive_loss(scores, train_n_passages)                                                                   Dense :134-140, ColBERT :154-160
    distill_loss(scores, teacher_scores, temperature)                                                            ColBERT/modeling.py:146-150

compute, with fused = lexical + lamb * semantic and the target of term k either P_k = softmax(teacher * temperature * teacher_split[k]) or,
without a teacher, the one-hot at column r * train_n_passages of row r,

    loss = (1 / R) sum_r [ weights[0] KL_r(fused, P_0) + weights[1] KL_r(semantic, P_1) + weights[2] KL_r(lexical, P_2) ]

in one launch plus a row sum.  The forward writes the loss, the fused scores (what `DHROutput.scores` returns) and, when an input requires a
gradient, dloss / dlexical and dloss / dsemantic for an upstream gradient of 1; only those are saved.  The backward multiplies them by the
upstream scalar with a torch op (this covers the reference's `loss * world_size`): it runs no library kernel and does not synchronise.

The loss and the returned scores are fp32; the scores carry no gradient path of their own (the reference's callers read them, they do not
differentiate through them).  Gradients come back in the dtype of the input they belong to.  fp16 and fp32 matrices, each on its own, are read
in place, row-strided views included; other dtypes are converted to fp32.  The inputs must be finite.  Every sum has a fixed order: two runs
on the same inputs are bit-identical.  Everything runs on the tensors' device and on torch's current stream.  There is no CPU implementation:
without the HIP library / a GPU the calls raise."""
from __future__ import annotations

import ctypes as C

from . import _lib
from . import _marshal as M

DHR_WEIGHTS, DHR_SPLIT = (1.0, 0.5, 0.5), (1.0, 0.75, 0.25)       # modeling.py:184-187: fused, semantic at 3/4, lexical at 1/4
FUSED_ONLY = (1.0, 0.0, 0.0)


def _read(t):
    """a [R, C] tensor, or None, as the kernel reads it: fp16 / fp32, row-strided views in place"""
    return None if t is None else M.as_read(M.values(t.detach()))[0]


def _arg(t):
    """(pointer, dtype code, row stride) of a prepared matrix, or of an absent one"""
    if t is None:
        return None, _lib.VAL_F32, 0
    return t.data_ptr(), _lib._val_code(t), M.lds(t)[0]


def _check(lexical, semantic, teacher, train_n_passages, lamb, temperature, weights, teacher_split):
    """Everything that can be refused before the library is touched.  -> (R, C, label_stride, weights, teacher_split)"""
    import torch
    for name, t in (("lexical_scores", lexical), ("semantic_scores", semantic), ("teacher_scores", teacher)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError("train loss: {} must be a torch tensor, got {}".format(name, type(t).__name__))
        if t.dim() != 2:
            raise ValueError("train loss: {} must be [queries, passages], got {} dimensions".format(name, t.dim()))
        if tuple(t.shape) != tuple(lexical.shape):
            raise RuntimeError("train loss: {} {} do not match lexical_scores {}".format(name, tuple(t.shape), tuple(lexical.shape)))
        if t.device != lexical.device:
            raise _lib.DhrError("train loss: {} live on {}, lexical_scores on {}: all scores must live on one device".format(name, t.device, lexical.device))
    weights, teacher_split = tuple(float(w) for w in weights), tuple(float(x) for x in teacher_split)
    if len(weights) != 3 or len(teacher_split) != 3:
        raise ValueError("train loss: weights and teacher_split hold three values each (fused, semantic, lexical)")
    if semantic is None and weights[1] != 0.0:
        raise ValueError("train loss: the semantic term has weight {} but there are no semantic scores".format(weights[1]))
    R, C_ = (int(d) for d in lexical.shape)
    n = int(train_n_passages)
    if teacher is not None:
        if not temperature > 0 or not all(x > 0 for x in teacher_split):
            raise ValueError("train loss: temperature {} and teacher_split {} must be positive".format(temperature, teacher_split))
    elif n < 0 or (R > 0 and C_ > 0 and (R - 1) * n >= C_):
        # the reference: RuntimeError from one_hot (class values must be smaller than num_classes)
        raise RuntimeError("train loss: train_n_passages = {} puts the label of query {} at column {}, outside {} passages".format(n, R - 1, (R - 1) * n, C_))
    return R, C_, n, weights, teacher_split


def _launch(lexical, semantic, teacher, R, C_, label_stride, lamb, temperature, weights, teacher_split, need_lex, need_sem):
    """prepared matrices -> (loss fp32 [], scores fp32 [R, C], dloss/dlexical or None, dloss/dsemantic or None)"""
    import torch
    dev = lexical.device
    scores = torch.empty((R, C_), dtype=torch.float32, device=dev)
    if R == 0 or C_ == 0:
        z = lambda t, need: torch.zeros((R, C_), dtype=t.dtype, device=dev) if need else None   # noqa: E731
        return torch.zeros((), dtype=torch.float32, device=dev), scores, z(lexical, need_lex), z(semantic, need_sem) if semantic is not None else None
    lib = _lib.load()
    loss = torch.empty((), dtype=torch.float32, device=dev)
    g_lex = torch.empty((R, C_), dtype=lexical.dtype, device=dev) if need_lex else None
    g_sem = torch.empty((R, C_), dtype=semantic.dtype, device=dev) if need_sem and semantic is not None else None
    kind = M.mem_kind(lexical)
    ws, ws_bytes = None, 0
    if kind == _lib.MEM_DEVICE:                       # the row losses come from torch's allocator: the library allocates nothing
        ws_bytes = int(lib.dhr_train_loss_workspace(R))
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    ptr = M.data_ptr
    _lib.check(lib.dhr_train_loss(M.device(lexical), kind, *_arg(lexical), *_arg(semantic), *_arg(teacher), R, C_, label_stride, float(lamb),
                                  float(temperature), (C.c_float * 3)(*weights), (C.c_float * 3)(*teacher_split), loss.data_ptr(), scores.data_ptr(), C_,
                                  ptr(g_lex), C_, ptr(g_sem), C_, ptr(ws), ws_bytes, M.stream(lexical)), "dhr_train_loss")
    return loss, scores, g_lex, g_sem


def _autograd_fn():
    """The torch.autograd.Function (built on first use, as in gip_scores.py)."""
    global _FN
    if _FN is not None:
        return _FN
    import torch

    class TrainLoss(torch.autograd.Function):
        @staticmethod
        def forward(ctx, lexical, semantic, teacher, cfg):
            R, C_, label_stride, lamb, temperature, weights, teacher_split = cfg
            need_lex = ctx.needs_input_grad[0]
            need_sem = semantic is not None and ctx.needs_input_grad[1]
            loss, scores, g_lex, g_sem = _launch(_read(lexical), _read(semantic), _read(teacher), R, C_, label_stride, lamb, temperature, weights,
                                                 teacher_split, need_lex, need_sem)
            ctx.save_for_backward(*(g for g in (g_lex, g_sem) if g is not None))
            ctx.have = (g_lex is not None, g_sem is not None)
            ctx.dtypes = (lexical.dtype, None if semantic is None else semantic.dtype)
            ctx.mark_non_differentiable(scores)
            ctx.set_materialize_grads(False)              # no zero-filled [R, C] gradient for the scores
            return loss, scores

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad_loss, _grad_scores):
            saved = list(ctx.saved_tensors)
            out = []
            if grad_loss is None:
                return None, None, None, None
            for have, dtype in zip(ctx.have, ctx.dtypes):
                if not have:
                    out.append(None)
                    continue
                g = saved.pop(0) * grad_loss.to(torch.float32)        # a 0-dim factor: the product keeps the gradient's own dtype
                out.append(g if g.dtype == dtype else g.to(dtype))
            return out[0], out[1], None, None

    _FN = TrainLoss
    return _FN


_FN = None


def hybrid_loss(lexical_scores, semantic_scores=None, teacher_scores=None, *, train_n_passages, lamb=1.0, temperature=1.0,
                weights=DHR_WEIGHTS, teacher_split=DHR_SPLIT):
    """-> (loss, scores): the fp32 scalar of the module docstring, differentiable with respect to lexical_scores and semantic_scores, and the
    fp32 fused scores lexical + lamb * semantic [R, C] (no gradient path).  weights = (fused, semantic, lexical); a term of weight 0 is not
    computed, and the semantic weight must be 0 without semantic_scores.  With teacher_scores [R, C] the targets are
    softmax(teacher * temperature * teacher_split[k]) (temperature and the splits positive) and train_n_passages is not used; without, the label
    of query r is column r * train_n_passages.  ValueError / RuntimeError for arguments the reference would fail on (shapes that do not match:
    RuntimeError; a label outside the columns: RuntimeError), DhrError for tensors on different devices."""
    import torch
    R, C_, label_stride, weights, teacher_split = _check(lexical_scores, semantic_scores, teacher_scores, train_n_passages, lamb, temperature,
                                                         weights, teacher_split)
    needs = torch.is_grad_enabled() and (lexical_scores.requires_grad or (semantic_scores is not None and semantic_scores.requires_grad))
    if needs:
        return _autograd_fn().apply(lexical_scores, semantic_scores, teacher_scores, (R, C_, label_stride, float(lamb), float(temperature), weights,
                                                                                     teacher_split))
    # nothing to differentiate: null gradient pointers
    loss, scores, _, _ = _launch(_read(lexical_scores), _read(semantic_scores), _read(teacher_scores), R, C_, label_stride, lamb, temperature,
                                 weights, teacher_split, False, False)
    return loss, scores


def dhr_loss(lexical_scores, semantic_scores, teacher_scores=None, *, train_n_passages, lamb, temperature=1.0):
    """The tail of DHRModel.forward in training (modeling.py:170-197) -> (loss, scores).  With teacher_scores (--tct: the teacher's
    listwise scores) the three KL terms of :184-187; without, the hard labels on the fused scores alone (:197)."""
    if semantic_scores is None:
        raise ValueError("dhr_loss: DHRModel.forward always fuses semantic scores (lamb = 0 switches them off)")
    return hybrid_loss(lexical_scores, semantic_scores, teacher_scores, train_n_passages=train_n_passages, lamb=lamb, temperature=temperature,
                       weights=DHR_WEIGHTS if teacher_scores is not None else FUSED_ONLY, teacher_split=DHR_SPLIT)


def aggretriever_loss(lexical_scores, semantic_scores=None, teacher_scores=None, *, train_n_passages, temperature=1.0):
    """The tail of the Aggretriever model's forward in training (Aggretriever/modeling.py:184-213) -> (loss, scores); scores = lexical +
    semantic.  With teacher_scores the three KL terms of :196-199 (they need semantic scores, as in the reference); with hard labels all
    three terms when semantic_scores is given (:208-211) and the fused term alone otherwise (:213)."""
    if teacher_scores is not None and semantic_scores is None:
        raise ValueError("aggretriever_loss: the distillation terms need semantic scores (the reference takes log_softmax of them)")
    return hybrid_loss(lexical_scores, semantic_scores, teacher_scores, train_n_passages=train_n_passages, lamb=1.0, temperature=temperature,
                       weights=DHR_WEIGHTS if semantic_scores is not None else FUSED_ONLY, teacher_split=DHR_SPLIT)


def contrastive_loss(scores, train_n_passages):
    """CrossEntropyLoss(mean) of [R, C] scores against the labels r * train_n_passages (Dense/modeling.py:134-140, ColBERT/modeling.py:154-160)
    -> the fp32 loss."""
    return hybrid_loss(scores, train_n_passages=train_n_passages, weights=FUSED_ONLY)[0]


def distill_loss(scores, teacher_scores, temperature=1.0):
    """ColBERT's KL against teacher scores (ColBERT/modeling.py:146-150): KLDivLoss(batchmean)(log_softmax(scores), softmax(teacher_scores *
    temperature)) -> the fp32 loss.  teacher_scores is [R, C]: the caller pads the teacher's [R, n] scores into the listwise layout as the
    reference does (with -20 after its own scaling, and temperature = 1 here; or unscaled with the temperature given here)."""
    return hybrid_loss(scores, None, teacher_scores, train_n_passages=1, temperature=temperature, weights=FUSED_ONLY, teacher_split=(1.0, 1.0, 1.0))[0]
