"""The gated inner product of a DHR / DLR training step and of the in-model reranker, differentiable, on the HIP ops `dhr_gip_scores`,
`dhr_gip_scores_backward` and `dhr_densify_backward`.

The reference (tevatron/DHR/modeling.py:250-285) densifies both sides, repeats the whole passage batch once per query, builds the
[n_q, n_p, dims] equality mask, multiplies and runs a batched matmul, and autograd keeps those tensors for the backward pass.  Here

    gip_scores(q_value, q_index, p_value, p_index, group=0)                          on densified arrays (the library's [value | index] records)
    listwise_gip_scores(q_reps, p_reps, effective_bsz, dims, remove_dims)            modeling.py:163 / :272-285
    pairwise_gip_scores(q_reps, p_reps, effective_bsz, train_n_passages, ...)        modeling.py:250-263
    paired_gip_scores(q_reps, p_reps, dims, remove_dims)                             modeling.py:215-218 (DHRModel.forward without training)

compute S[b][p] = sum_d (q_index[b][d] == p_index[p][d]) * q_value[b][d] * p_value[p][d] without any [n_q, n_p, dims] temporary, and
`.backward()` runs scores backward -> densify backward, so the gradient arrives in `q_reps.grad` / `p_reps.grad` ([B, V], zero outside the one
column per slice that densify picked: first group on ties).

Scores are fp32 always.  Under `torch.autocast` the reference's matmul would return fp16; returning the unrounded fp32 sums is deliberate
(the loss that follows is computed in fp32 anyway).  Gradients come back in the dtype of the input they belong to.  Every sum has a fixed
order: two runs on the same inputs are bit-identical.

Torch CUDA tensors are processed on their device and on torch's current stream, without a host synchronisation; numpy arrays (and torch CPU
tensors) are staged through device 0.  There is no CPU implementation: without the HIP library / a GPU the calls raise."""
from __future__ import annotations

import numpy as np

from . import _lib
from . import _marshal as M
from .densify import _check as _densify_check


def _prepare(q_value, q_index, p_value, p_index, group):
    """Common dtypes and row-strided 2-D views of the four arrays; shape checks.  -> (qv, qi, pv, pi, n_q, n_p, dims)."""
    arrays = (q_value, q_index, p_value, p_index)
    if len({M.is_np(a) for a in arrays}) != 1:
        raise TypeError("gip_scores: numpy arrays and torch tensors cannot be mixed")
    if not M.is_np(q_value):
        q_value, q_index, p_value, p_index = (a.detach() for a in arrays)
        if len({a.device for a in (q_value, q_index, p_value, p_index)}) != 1:
            raise _lib.DhrError("gip_scores: all four tensors must live on one device")
    for a, b, what in ((q_value, q_index, "query"), (p_value, p_index, "passage")):
        if len(a.shape) != 2 or tuple(a.shape) != tuple(b.shape):
            raise ValueError("gip_scores: {} values {} and indices {} must be [rows, dims] of one shape".format(what, tuple(a.shape), tuple(b.shape)))
    n_q, dims = (int(d) for d in q_value.shape)
    n_p = int(p_value.shape[0])
    if int(p_value.shape[1]) != dims:
        raise RuntimeError("gip_scores: queries have {} dims, passages {}".format(dims, int(p_value.shape[1])))
    if group < 0 or (group > 0 and n_p != n_q * group):
        raise RuntimeError("gip_scores: {} passage rows for {} queries x {} passages per query".format(n_p, n_q, group))
    vname = M.common_dtype(q_value, p_value, M.FLOATS, "float32")
    iname = M.common_dtype(q_index, p_index, M.NARROW, "int16")                # (int64 of densify() is narrowed: groups < 32768)
    qv, qi, pv, pi = (M.as_read(M.cast(a, name))[0] for a, name in ((q_value, vname), (q_index, iname), (p_value, vname), (p_index, iname)))
    return qv, qi, pv, pi, n_q, n_p, dims


def _sides(qv, qi, pv, pi, n_q, n_p):
    (ld_qv,), (ld_qi,), (ld_pv,), (ld_pi,) = (M.lds(a) for a in (qv, qi, pv, pi))
    return M.mem_kind(qv), (M.data_ptr(qv), ld_qv, M.data_ptr(qi), ld_qi, n_q, M.data_ptr(pv), ld_pv, M.data_ptr(pi), ld_pi, n_p)


def _forward(qv, qi, pv, pi, n_q, n_p, dims, group):
    """prepared arrays -> fp32 scores [n_q, n_p] (listwise) / [n_q, group]."""
    lib = _lib.load()
    out = M.empty(qv, (n_q, group if group > 0 else n_p), "float32")
    if n_q == 0 or n_p == 0:
        return out
    kind, sides = _sides(qv, qi, pv, pi, n_q, n_p)
    ws, ws_bytes = None, 0
    if kind == _lib.MEM_DEVICE:                       # the workspace of a split over dims comes from torch's allocator
        ws_bytes = int(lib.dhr_gip_scores_workspace(n_q, n_p, dims, group))
        if ws_bytes:
            ws = M.empty(qv, (ws_bytes,), "uint8")
    p_out, ld_out, _ = _lib._ptr_ld(out)
    _lib.check(lib.dhr_gip_scores(M.device(qv), kind, *sides, dims, _lib._val_code(qv), _lib.idx_code(qi.dtype), group, p_out, ld_out,
                                  None if ws is None else ws.data_ptr(), ws_bytes, M.stream(qv)), "dhr_gip_scores")
    return out


def _backward(qv, qi, pv, pi, n_q, n_p, dims, group, grad, need_q, need_p):
    """-> (dL/dq_value, dL/dp_value) fp32, None where not needed.  grad: (fp32 [n_q, cols], row stride) as M.grad_rows returns it."""
    lib = _lib.load()
    dq = M.empty(qv, (n_q, dims), "float32") if need_q else None
    dp = M.empty(qv, (n_p, dims), "float32") if need_p else None
    if not (need_q or need_p):
        return dq, dp
    kind, sides = _sides(qv, qi, pv, pi, n_q, n_p)
    grad, ld_g = grad
    if M.mem_kind(grad) != kind:
        raise _lib.DhrError("gip_scores backward: the gradient must live in the same memory kind as the inputs")
    p_dq, ld_dq = (None, 0) if dq is None else _lib._ptr_ld(dq)[:2]
    p_dp, ld_dp = (None, 0) if dp is None else _lib._ptr_ld(dp)[:2]
    _lib.check(lib.dhr_gip_scores_backward(M.device(qv), kind, *sides, dims, _lib._val_code(qv), _lib.idx_code(qi.dtype), group, M.data_ptr(grad), ld_g,
                                           p_dq, ld_dq, p_dp, ld_dp, M.stream(qv)), "dhr_gip_scores_backward")
    return dq, dp


def _densify_fwd(reps, dims, remove_dims):
    """[B, V] fp16 / fp32 reps -> (fp32 values [B, dims], uint8 / int16 groups [B, dims]) on dhr_densify (exact values, first group on ties)."""
    import torch
    lib = _lib.load()
    B, V = int(reps.shape[0]), int(reps.shape[1])
    src, (ld_in,) = M.as_read(M.values(reps.detach()))
    val = torch.empty((B, dims), dtype=torch.float32, device=src.device)
    idx = torch.empty((B, dims), dtype=torch.int16 if (V - remove_dims) // dims > 256 else torch.uint8, device=src.device)
    if B:
        _lib.check(lib.dhr_densify(M.device(src), M.mem_kind(src), src.data_ptr(), _lib._val_code(src), ld_in, B, V, remove_dims, dims, val.data_ptr(),
                                   _lib.VAL_F32, dims, idx.data_ptr(), _lib.idx_code(idx.dtype), dims, M.stream(src)), "dhr_densify")
    return val, idx


def _densify_bwd(dval, idx, vocab, dims, remove_dims, dtype):
    """fp32 dL/dvalue [B, dims] + groups -> the whole dL/dreps [B, vocab] in `dtype` (fp16 / fp32), written in one pass."""
    import torch
    lib = _lib.load()
    B = int(dval.shape[0])
    out_dtype = dtype if dtype in (torch.float16, torch.float32) else torch.float32
    out = torch.empty((B, vocab), dtype=out_dtype, device=dval.device)
    if B:
        _lib.check(lib.dhr_densify_backward(M.device(dval), M.mem_kind(dval), dval.data_ptr(), dval.stride(0), idx.data_ptr(), _lib.idx_code(idx.dtype),
                                            idx.stride(0), B, vocab, remove_dims, dims, out.data_ptr(), _lib._val_code(out), vocab, M.stream(dval)),
                   "dhr_densify_backward")
    return out if out_dtype == dtype else out.to(dtype)


def _autograd_fns():
    """The two torch.autograd.Functions (built on first use: numpy callers never import torch through this module)."""
    global _FNS
    if _FNS is not None:
        return _FNS
    import torch

    class GipScores(torch.autograd.Function):
        @staticmethod
        def forward(ctx, q_value, q_index, p_value, p_index, group):
            qv, qi, pv, pi, n_q, n_p, dims = _prepare(q_value, q_index, p_value, p_index, group)
            ctx.save_for_backward(qv, qi, pv, pi)
            ctx.geom = (n_q, n_p, dims, group, q_value.dtype, p_value.dtype)
            return _forward(qv, qi, pv, pi, n_q, n_p, dims, group)

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad):
            qv, qi, pv, pi = ctx.saved_tensors
            n_q, n_p, dims, group, q_dtype, p_dtype = ctx.geom
            dq, dp = _backward(qv, qi, pv, pi, n_q, n_p, dims, group, M.grad_rows(grad, n_q, group if group > 0 else n_p), ctx.needs_input_grad[0],
                               ctx.needs_input_grad[2])
            return (None if dq is None else dq.to(q_dtype)), None, (None if dp is None else dp.to(p_dtype)), None, None

    class FusedGipScores(torch.autograd.Function):
        @staticmethod
        def forward(ctx, q_reps, p_reps, dims, remove_dims, group):
            qv, qi = _densify_fwd(q_reps, dims, remove_dims)
            pv, pi = _densify_fwd(p_reps, dims, remove_dims)
            n_q, n_p = int(qv.shape[0]), int(pv.shape[0])
            ctx.save_for_backward(qv, qi, pv, pi)
            ctx.geom = (n_q, n_p, dims, remove_dims, group, int(q_reps.shape[1]), int(p_reps.shape[1]), q_reps.dtype, p_reps.dtype)
            return _forward(qv, qi, pv, pi, n_q, n_p, dims, group)

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad):
            qv, qi, pv, pi = ctx.saved_tensors
            n_q, n_p, dims, remove_dims, group, q_vocab, p_vocab, q_dtype, p_dtype = ctx.geom
            dq, dp = _backward(qv, qi, pv, pi, n_q, n_p, dims, group, M.grad_rows(grad, n_q, group if group > 0 else n_p), ctx.needs_input_grad[0],
                               ctx.needs_input_grad[1])
            gq = None if dq is None else _densify_bwd(dq, qi, q_vocab, dims, remove_dims, q_dtype)
            del dq
            gp = None if dp is None else _densify_bwd(dp, pi, p_vocab, dims, remove_dims, p_dtype)
            return gq, gp, None, None, None

    _FNS = (GipScores, FusedGipScores)
    return _FNS


_FNS = None


def gip_scores(q_value, q_index, p_value, p_index, group: int = 0):
    """Gated inner products of densified arrays: values [n_q, dims] / [n_p, dims] (fp16 or fp32; a [:, :dims] view of a record is read in
    place), group indices of any integer dtype (int64 from densify() is narrowed to int16).  group = 0: every query against every passage,
    -> fp32 [n_q, n_p]; group = n > 0: passage row b * n + j belongs to query b, -> fp32 [n_q, n].  numpy in -> numpy out; torch in -> torch
    out on the same device, differentiable with respect to the two value tensors."""
    group = int(group)
    if M.is_np(q_value):
        qv, qi, pv, pi, n_q, n_p, dims = _prepare(q_value, q_index, p_value, p_index, group)
        return _forward(qv, qi, pv, pi, n_q, n_p, dims, group)
    return _autograd_fns()[0].apply(q_value, q_index, p_value, p_index, group)


def _fused(q_reps, p_reps, dims, remove_dims, group):
    if M.is_np(q_reps) or M.is_np(p_reps):
        from .densify import densify
        qv, qi = densify(np.asarray(q_reps), dims, remove_dims=remove_dims)
        pv, pi = densify(np.asarray(p_reps), dims, remove_dims=remove_dims)
        return gip_scores(qv, qi, pv, pi, group)
    if q_reps.device != p_reps.device:
        raise _lib.DhrError("gip scores: query and passage reps must live on one device")
    return _autograd_fns()[1].apply(q_reps, p_reps, int(dims), int(remove_dims), int(group))


def _squeeze(scores):
    return np.squeeze(scores) if M.is_np(scores) else scores.squeeze()


def listwise_gip_scores(q_reps, p_reps, effective_bsz: int, dims: int = 768, remove_dims: int = 570):
    """DHRModel.listwise_gip_scores (modeling.py:272-285) on [B, V] lexical reps: every query against every passage of the batch.  Returns
    what the reference returns, its .squeeze() included ([effective_bsz, P]; [P] for one query, [effective_bsz] for one passage), in fp32.
    ValueError as densify raises it; RuntimeError where the query rows are not effective_bsz (the reference's view / broadcast fails)."""
    n_q, _ = _densify_check(q_reps, dims, remove_dims)
    n_p, _ = _densify_check(p_reps, dims, remove_dims)
    if n_q != int(effective_bsz):
        raise RuntimeError("listwise_gip_scores: query reps {} do not hold effective_bsz = {} rows (passage reps {})".format(
            tuple(q_reps.shape), effective_bsz, tuple(p_reps.shape)))
    return _squeeze(_fused(q_reps, p_reps, dims, remove_dims, 0).reshape(n_q, 1, n_p))


def pairwise_gip_scores(q_reps, p_reps, effective_bsz: int, train_n_passages: int, dims: int = 768, remove_dims: int = 570):
    """DHRModel.pairwise_gip_scores (modeling.py:250-263): query b against its own passages, rows b * train_n_passages + j of p_reps.
    -> fp32 [effective_bsz, train_n_passages], squeezed like the reference.  RuntimeError where the rows do not fit that layout."""
    n_q, _ = _densify_check(q_reps, dims, remove_dims)
    n_p, _ = _densify_check(p_reps, dims, remove_dims)
    if n_q != int(effective_bsz) or int(train_n_passages) <= 0 or n_p != n_q * int(train_n_passages):
        raise RuntimeError("pairwise_gip_scores: query reps {} and passage reps {} are not effective_bsz = {} queries x train_n_passages = {} "
                           "passages".format(tuple(q_reps.shape), tuple(p_reps.shape), effective_bsz, train_n_passages))
    return _squeeze(_fused(q_reps, p_reps, dims, remove_dims, int(train_n_passages)).reshape(n_q, 1, int(train_n_passages)))


def paired_gip_scores(q_reps, p_reps, dims: int = 768, remove_dims: int = 570):
    """The lexical score of DHRModel.forward outside training (modeling.py:215-218; the reranker of tevatron/driver/eval.py): row i of q_reps
    against row i of p_reps -> fp32 [B].  One row on either side broadcasts against the other, as in the reference."""
    n_q, _ = _densify_check(q_reps, dims, remove_dims)
    n_p, _ = _densify_check(p_reps, dims, remove_dims)
    if n_q != n_p and n_q != 1 and n_p != 1:
        raise RuntimeError("paired_gip_scores: query reps {} and passage reps {} neither pair up nor broadcast".format(tuple(q_reps.shape), tuple(p_reps.shape)))
    return _fused(q_reps, p_reps, dims, remove_dims, 1 if n_q == n_p else 0).reshape(max(n_q, n_p))
