"""Late-interaction (MaxSim) scores of a ColBERT training step and of the TCT teacher of a DHR step, differentiable, on the HIP ops
`dhr_maxsim_scores` and `dhr_maxsim_scores_backward`.

The reference (tevatron/ColBERT/modeling.py:204-219, :188-190) builds einsum('aik,bjk->abij') as one [n_q, n_p, Lq, Lp] tensor, takes the
max over passage tokens and the sum over query tokens, and autograd keeps that tensor and scatters into a zero-filled copy of it.  Here

    maxsim_scores(q, p, group=0)                                   the primitive on [A, Lq, D] / [B, Lp, D] token vectors
    listwise_maxsim(q_seq_reps, p_seq_reps)                        modeling.py:214-219 (and the [A, 1, D] CLS call at :141)
    pairwise_maxsim(q_seq_reps, p_seq_reps, train_n_passages)      modeling.py:204-212
    paired_maxsim(q_seq_reps, p_seq_reps)                          modeling.py:188-189 (ColBERT.forward outside training, no teacher)

compute S[a][b] = sum_i max_j <q[a][i], p[b][j]> without that tensor: the forward keeps the int16 token that won each maximum (the first
on ties, as torch.max on the CPU), the backward routes dL/dS through it.  There is no mask argument: the reference multiplies padded
tokens to zero vectors and lets them take part with similarity 0, and so does this.

Scores are fp32 always (under `torch.autocast` the reference would return fp16; returning the unrounded fp32 sums is deliberate).  Gradients
come back in the dtype of the input they belong to.  Every sum has a fixed order: two runs on the same inputs are bit-identical, and
`group = n` equals the matching entries of `group = 0` bit for bit.  Token and batch strides are free (a `reps[:, 1:]` view is read in place);
only the last dimension must be contiguous.  Without a gradient to compute (no input requires one, or under `torch.no_grad()`) the winning
tokens are neither allocated nor stored.

Torch CUDA tensors are processed on their device and on torch's current stream, without a host synchronisation; numpy arrays (and torch CPU
tensors) are staged through device 0, forward only for numpy.  There is no CPU implementation: without the HIP library / a GPU the calls
raise."""
from __future__ import annotations

import numpy as np

from . import _lib
from . import _marshal as M

MAX_DIMS, MAX_PASSAGE_TOKENS = 1024, 32767


def _side(a):
    """(pointer, token stride, batch stride) of a prepared [n, L, D] operand"""
    st, sb = M.lds(a)[::-1]
    return M.data_ptr(a), st, sb


def _prepare(q, p, group):
    """Shape checks, one common kernel dtype, strided 3-D views.  -> (q, p, A, B, Lq, Lp, D, cols)"""
    if M.is_np(q) != M.is_np(p):
        raise TypeError("maxsim_scores: numpy arrays and torch tensors cannot be mixed")
    if len(q.shape) != 3 or len(p.shape) != 3:
        raise ValueError("maxsim_scores: token vectors must be [batch, tokens, dims], got {} and {}".format(tuple(q.shape), tuple(p.shape)))
    A, Lq, D = (int(d) for d in q.shape)
    B, Lp, Dp = (int(d) for d in p.shape)
    if D != Dp:
        raise RuntimeError("maxsim_scores: queries have {} dims, passages {}".format(D, Dp))
    if group < 0 or (group > 0 and B != A * group):
        raise RuntimeError("maxsim_scores: {} passage rows for {} queries x {} passages per query".format(B, A, group))
    if Lq < 1 or Lp < 1 or D < 1:
        raise ValueError("maxsim_scores: empty token or dims axis: {} and {}".format(tuple(q.shape), tuple(p.shape)))
    if D > MAX_DIMS or Lp > MAX_PASSAGE_TOKENS:
        raise _lib.DhrError("maxsim_scores: at most {} dims and {} passage tokens are supported, got {} and {}".format(MAX_DIMS, MAX_PASSAGE_TOKENS, D, Lp),
                            status=_lib.ERR_UNSUPPORTED)
    if not M.is_np(q):
        q, p = q.detach(), p.detach()
        if q.device != p.device:
            raise _lib.DhrError("maxsim_scores: query and passage vectors must live on one device")
    name = M.common_dtype(q, p, M.FLOATS, "float32")
    # the library reads any token and batch stride >= D in place (batches may overlap); anything else is copied once
    q, p = (M.as_read(M.cast(a, name), disjoint=False)[0] for a in (q, p))
    return q, p, A, B, Lq, Lp, D, (group if group > 0 else B)


def _forward(q, p, A, B, Lq, Lp, D, cols, group, want_arg):
    """prepared arrays -> (fp32 scores [A, cols], int16 winners [A, cols, Lq] or None)"""
    out = M.empty(q, (A, cols), "float32")
    arg = M.empty(q, (A, cols, Lq), "int16") if want_arg else None
    if A == 0 or B == 0:
        return out, arg
    lib = _lib.load()
    (pq, q_tok, q_batch), (pp, p_tok, p_batch), kind = _side(q), _side(p), M.mem_kind(q)
    if kind != M.mem_kind(p):
        raise _lib.DhrError("maxsim_scores: query and passage vectors must live in the same memory kind")
    _lib.check(lib.dhr_maxsim_scores(M.device(q), kind, pq, q_tok, q_batch, A, Lq, pp, p_tok, p_batch, B, Lp, D, _lib._val_code(q), group,
                                     M.data_ptr(out), cols, M.data_ptr(arg), M.stream(q)), "dhr_maxsim_scores")
    return out, arg


def _backward(q, p, A, B, Lq, Lp, D, cols, group, arg, grad, need_q, need_p, q_dtype, p_dtype):
    """-> (dL/dq [A, Lq, D], dL/dp [B, Lp, D]) in the inputs' own dtypes, None where not needed.
    grad: (fp32 [A, cols], row stride) as M.grad_rows returns it."""
    import torch
    lib = _lib.load()
    # the kernels write fp32, or fp16 rounded once; any other input dtype gets its gradient converted from fp32
    code = _lib.VAL_F16 if q.dtype == torch.float16 else _lib.VAL_F32
    dq = torch.empty((A, Lq, D), dtype=q.dtype, device=q.device) if need_q else None
    dp = torch.empty((B, Lp, D), dtype=q.dtype, device=q.device) if need_p else None
    if need_q or need_p:
        (pq, q_tok, q_batch), (pp, p_tok, p_batch), kind = _side(q), _side(p), M.mem_kind(q)
        _lib.check(lib.dhr_maxsim_scores_backward(M.device(q), kind, pq, q_tok, q_batch, A, Lq, pp, p_tok, p_batch, B, Lp, D, _lib._val_code(q), group,
                                                  arg.data_ptr(), grad[0].data_ptr(), grad[1], M.data_ptr(dq), M.data_ptr(dp), code, M.stream(q)),
                   "dhr_maxsim_scores_backward")
    return (None if dq is None else dq.to(q_dtype)), (None if dp is None else dp.to(p_dtype))


def _autograd_fn():
    """The torch.autograd.Function (built on first use: numpy callers never import torch through this module)."""
    global _FN
    if _FN is not None:
        return _FN
    import torch

    class MaxSimScores(torch.autograd.Function):
        @staticmethod
        def forward(ctx, q, p, group):
            qq, pp, A, B, Lq, Lp, D, cols = _prepare(q, p, group)
            out, arg = _forward(qq, pp, A, B, Lq, Lp, D, cols, group, True)
            ctx.save_for_backward(qq, pp, arg)
            ctx.geom = (A, B, Lq, Lp, D, cols, group, q.dtype, p.dtype)
            return out

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad):
            qq, pp, arg = ctx.saved_tensors
            A, B, Lq, Lp, D, cols, group, q_dtype, p_dtype = ctx.geom
            if A == 0 or B == 0:
                z = lambda n, L, dt, need: torch.zeros((n, L, D), dtype=dt, device=qq.device) if need else None   # noqa: E731
                return z(A, Lq, q_dtype, ctx.needs_input_grad[0]), z(B, Lp, p_dtype, ctx.needs_input_grad[1]), None
            dq, dp = _backward(qq, pp, A, B, Lq, Lp, D, cols, group, arg, M.grad_rows(grad, A, cols), ctx.needs_input_grad[0], ctx.needs_input_grad[1],
                               q_dtype, p_dtype)
            return dq, dp, None

    _FN = MaxSimScores
    return _FN


_FN = None


def maxsim_scores(q, p, group: int = 0):
    """S[a][b] = sum_i max_j <q[a][i], p[b][j]> for q [A, Lq, D] and p [B, Lp, D] (fp16 or fp32 are read in place; bf16 and other dtypes are
    converted to fp32, which is exact, and mixed fp16 / fp32 goes to fp32).  group = 0: every pair, -> fp32 [A, B]; group = n > 0: passage
    row a * n + j belongs to query a, -> fp32 [A, n].  numpy in -> numpy out (forward only); torch in -> torch out on the same device,
    differentiable with respect to both."""
    group = int(group)
    if not (M.is_np(q) or M.is_np(p)):
        import torch
        if torch.is_grad_enabled() and (q.requires_grad or p.requires_grad):
            return _autograd_fn().apply(q, p, group)
    qq, pp, A, B, Lq, Lp, D, cols = _prepare(q, p, group)            # nothing to differentiate: no winners are kept
    return _forward(qq, pp, A, B, Lq, Lp, D, cols, group, False)[0]


def _check3d(q, p, what):
    if len(q.shape) != 3 or len(p.shape) != 3:
        raise ValueError("{}: token vectors must be [batch, tokens, dims], got {} and {}".format(what, tuple(q.shape), tuple(p.shape)))
    if int(q.shape[2]) != int(p.shape[2]):
        raise RuntimeError("{}: queries have {} dims, passages {}".format(what, int(q.shape[2]), int(p.shape[2])))


def _squeeze(scores):
    return np.squeeze(scores) if M.is_np(scores) else scores.squeeze()


def listwise_maxsim(q_seq_reps, p_seq_reps):
    """ColBERT.listwise_maxsim (modeling.py:214-219): every query against every passage, -> fp32 [A, B], no squeeze.  The [A, 1, D] CLS
    vectors of modeling.py:141 go through the same call.  RuntimeError where the dims differ (the reference's einsum fails)."""
    _check3d(q_seq_reps, p_seq_reps, "listwise_maxsim")
    return maxsim_scores(q_seq_reps, p_seq_reps, 0)


def pairwise_maxsim(q_seq_reps, p_seq_reps, train_n_passages: int):
    """ColBERT.pairwise_maxsim (modeling.py:204-212): query a against its own passages, rows a * train_n_passages + j of p_seq_reps.
    -> fp32 [A, train_n_passages], squeezed like the reference ([n] for one query, [A] for one passage each).  RuntimeError where the rows
    do not form A x train_n_passages (the reference's view fails)."""
    _check3d(q_seq_reps, p_seq_reps, "pairwise_maxsim")
    n = int(train_n_passages)
    if n <= 0 or int(p_seq_reps.shape[0]) != int(q_seq_reps.shape[0]) * n:
        raise RuntimeError("pairwise_maxsim: passage vectors {} are not {} queries x train_n_passages = {} passages".format(
            tuple(p_seq_reps.shape), int(q_seq_reps.shape[0]), train_n_passages))
    return _squeeze(maxsim_scores(q_seq_reps, p_seq_reps, n))


def paired_maxsim(q_seq_reps, p_seq_reps):
    """The token score of ColBERT.forward outside training without a teacher (modeling.py:188-189): row a of q_seq_reps against row a of
    p_seq_reps, -> fp32 [A].  RuntimeError where the rows do not pair up."""
    _check3d(q_seq_reps, p_seq_reps, "paired_maxsim")
    if int(q_seq_reps.shape[0]) != int(p_seq_reps.shape[0]):
        raise RuntimeError("paired_maxsim: query vectors {} and passage vectors {} do not pair up".format(tuple(q_seq_reps.shape), tuple(p_seq_reps.shape)))
    return maxsim_scores(q_seq_reps, p_seq_reps, 1).reshape(int(q_seq_reps.shape[0]))
