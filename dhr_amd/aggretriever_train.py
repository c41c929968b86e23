"""The two stretches of an Aggretriever TRAINING step that follow the encoder, differentiable, on the HIP ops `dhr_aggregate_train` /
`dhr_aggregate_backward` and `dhr_term_weight_head` / `dhr_term_weight_head_backward` (dhr_amd/csrc/aggretriever_train.hip).

The reference (tevatron/Aggretriever/utils.py:16-44 at modeling.py:173-174; --skip_mlm at modeling.py:279-284, 311-316) runs, in eager torch
with autograd on,

    tok_reps = aggregate(lexical_reps, agg_dim, full=...)          # a pad or slice copy of [B, V], a max with int64 indices, two strided slices,
                                                                   # two masks, three products; the backward scatters into zero-filled copies
    reps = torch.zeros(B, L, 30522, dtype=hidden.dtype)            # 3.5 GB in fp32 at 192 passages x 150 tokens
    reps = torch.scatter(reps, dim=-1, index=input_ids[:, 1:, None], src=term_weights).max(-2).values

Here

    aggregate(lexical_reps, dims=640, full=True, return_route=False)                             -> [B, dims]        (or (out, route))
    term_weight_reps(input_ids, term_weights, vocab=30522, skip_tokens=1, return_tokens=False)   -> [B, vocab] fp32  (or (reps, tok))

keep, besides their inputs and outputs, one int16 per output column (`route`) and one int16 per vocabulary column (`tok`).  Both are
selections: every output and every gradient entry is an input value, its negation or zero, so they equal the reference's exactly.
`aggregate(term_weight_reps(...))` and `aggregate(lexical_train.lexical_reps(...))` are the two Aggretriever encoders.

Everything is enqueued on torch's current stream of the inputs' device, without a host synchronisation; buffers come from torch's allocator.
There is no CPU implementation: without a GPU the calls raise."""
from __future__ import annotations

from . import _lib
from . import _marshal as M
from .lexical import VOCAB_SIZE, _agg_geometry

MAX_TOKENS, MAX_GROUPS = 32767, 16383


def _check_aggregate(lexical_reps, dims, full):
    """Shape / dtype / device checks, before the library is touched.  -> (B, V, remove)"""
    import torch
    if not isinstance(lexical_reps, torch.Tensor):
        raise _lib.DhrError("aggretriever_train.aggregate: a torch tensor on a GPU is required (dhr_amd.lexical.aggregate serves numpy arrays, without gradients)")
    if lexical_reps.dim() != 2:
        raise ValueError('Input lexical representation shape should be 2 (batch, vocab), but the input shape is {}'.format(lexical_reps.dim()))
    B, V = (int(d) for d in lexical_reps.shape)
    remove, width = _agg_geometry(B, V, dims, full)
    if lexical_reps.dtype not in (torch.float16, torch.float32):
        raise _lib.DhrError(f"unsupported lexical reps dtype {lexical_reps.dtype} (float16 / float32)")
    if (V - remove) // width > MAX_GROUPS:
        raise _lib.DhrError("aggretriever_train.aggregate: more than {} groups".format(MAX_GROUPS), status=_lib.ERR_UNSUPPORTED)
    if not lexical_reps.is_cuda:
        raise _lib.DhrError("aggretriever_train.aggregate: the lexical reps must live on a GPU (there is no CPU implementation)")
    return B, V, remove


def _check_term_weights(input_ids, term_weights, vocab, skip_tokens):
    """Shape / dtype / device checks, before the library is touched.  -> (B, L, T)"""
    import torch
    if not isinstance(input_ids, torch.Tensor) or not isinstance(term_weights, torch.Tensor):
        raise _lib.DhrError("aggretriever_train.term_weight_reps: torch tensors on a GPU are required")
    if input_ids.dim() != 2:
        raise ValueError('input_ids must be [batch, tokens], got {} dimensions'.format(input_ids.dim()))
    B, L = (int(d) for d in input_ids.shape)
    if skip_tokens < 0:
        raise ValueError('skip_tokens must be >= 0, got {}'.format(skip_tokens))
    T = L - skip_tokens
    if T <= 0:
        raise ValueError('no tokens: the maximum over tokens of an empty sequence is undefined ({} tokens, {} skipped)'.format(L, skip_tokens))
    if vocab <= 0:
        raise ValueError('vocab must be > 0, got {}'.format(vocab))
    if tuple(term_weights.shape) not in ((B, T), (B, T, 1)):
        raise ValueError('term_weights must be [{}, {}] or [{}, {}, 1] (batch, tokens - skip_tokens), got {}'.format(B, T, B, T, tuple(term_weights.shape)))
    if T > MAX_TOKENS:
        raise ValueError('more than {} tokens'.format(MAX_TOKENS))
    if input_ids.dtype not in (torch.int32, torch.int64):
        raise _lib.DhrError(f"unsupported input_ids dtype {input_ids.dtype} (int32 / int64)")
    if term_weights.dtype not in (torch.float16, torch.float32):
        raise _lib.DhrError(f"unsupported term_weights dtype {term_weights.dtype} (float16 / float32)")
    if not term_weights.is_cuda:
        raise _lib.DhrError("aggretriever_train.term_weight_reps: the term weights must live on a GPU (there is no CPU implementation)")
    if input_ids.device != term_weights.device:
        raise _lib.DhrError("aggretriever_train.term_weight_reps: input_ids and term_weights must live on one device")
    return B, L, T


def _functions():
    """The two torch.autograd.Functions (built on first use, like dhr_amd.lexical_train)."""
    global _FNS
    if _FNS is not None:
        return _FNS
    import torch

    class Aggregate(torch.autograd.Function):
        @staticmethod
        def forward(ctx, reps, dims, full):
            B, V, remove = _check_aggregate(reps, dims, full)
            lib = _lib.load()
            x, (ld_x,) = M.as_read(reps.detach())
            out = torch.empty((B, dims), dtype=x.dtype, device=x.device)
            route = torch.empty((B, dims), dtype=torch.int16, device=x.device)
            code = _lib._val_code(x)
            _lib.check(lib.dhr_aggregate_train(M.device(x), _lib.MEM_DEVICE, x.data_ptr(), code, ld_x, B, V, dims, remove, 1 if full else 0,
                                               out.data_ptr(), code, dims, route.data_ptr(), dims, M.stream(x)), "dhr_aggregate_train")
            ctx.save_for_backward(route)
            ctx.geom = (B, V, dims, remove, full, x.dtype)
            ctx.mark_non_differentiable(route)
            return out, route

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad, _grad_route):
            route, = ctx.saved_tensors
            B, V, dims, remove, full, dtype = ctx.geom
            if not ctx.needs_input_grad[0]:
                return None, None, None
            lib = _lib.load()
            g, ld_g = M.grad_rows(grad, B, dims, dtype)
            dx = torch.empty((B, V), dtype=dtype, device=route.device)
            _lib.check(lib.dhr_aggregate_backward(M.device(route), _lib.MEM_DEVICE, g.data_ptr(), _lib._val_code(g), ld_g,
                                                  route.data_ptr(), dims, B, V, dims, remove, 1 if full else 0, dx.data_ptr(), V, M.stream(dx)),
                       "dhr_aggregate_backward")
            return dx, None, None

    class TermWeightReps(torch.autograd.Function):
        @staticmethod
        def forward(ctx, input_ids, term_weights, vocab, skip_tokens):
            B, L, T = _check_term_weights(input_ids, term_weights, vocab, skip_tokens)
            lib = _lib.load()
            ids, (ld_ids,) = M.as_read(input_ids.detach())
            w, (ld_w,) = M.as_read(term_weights.detach().reshape(B, T))
            reps = torch.empty((B, vocab), dtype=torch.float32, device=w.device)
            tok = torch.empty((B, vocab), dtype=torch.int16, device=w.device)
            if B:
                _lib.check(lib.dhr_term_weight_head(M.device(w), _lib.MEM_DEVICE, ids.data_ptr(), ids.element_size(), ld_ids, w.data_ptr(),
                                                    _lib._val_code(w), ld_w, B, T, skip_tokens, vocab, reps.data_ptr(), vocab, tok.data_ptr(),
                                                    vocab, M.stream(w)), "dhr_term_weight_head")
            ctx.save_for_backward(ids, tok)
            ctx.geom = (B, L, T, vocab, skip_tokens, tuple(term_weights.shape), term_weights.dtype)
            ctx.mark_non_differentiable(tok)
            return reps, tok

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad, _grad_tok):
            ids, tok = ctx.saved_tensors
            B, L, T, vocab, skip_tokens, w_shape, w_dtype = ctx.geom
            if not ctx.needs_input_grad[1]:
                return None, None, None, None
            lib = _lib.load()
            g, ld_g = M.grad_rows(grad, B, vocab)
            dw = torch.empty((B, T), dtype=w_dtype, device=tok.device)
            if B:
                _lib.check(lib.dhr_term_weight_head_backward(M.device(tok), _lib.MEM_DEVICE, ids.data_ptr(), ids.element_size(), M.lds(ids)[0], B, T,
                                                             skip_tokens, vocab, g.data_ptr(), ld_g, tok.data_ptr(), vocab, dw.data_ptr(),
                                                             _lib._val_code(dw), T, M.stream(dw)), "dhr_term_weight_head_backward")
            return None, dw.reshape(w_shape), None, None

    _FNS = (Aggregate, TermWeightReps)
    return _FNS


_FNS = None


def aggregate(lexical_reps, dims: int = 640, full: bool = True, return_route: bool = False):
    """tevatron/Aggretriever/utils.py:16-44 with `.backward()`: [B, V] reps (fp16 or fp32, any row stride, the last dimension contiguous) ->
    [B, dims] in the reps' dtype, bit-identical to `dhr_amd.lexical.aggregate`.  full=True removes cal_remove_dim(2 * dims) leading columns
    (a negative value pads that many zero columns at the end) and folds groups of 2 * dims columns into pos * (pos > neg) - neg * (pos <= neg)
    of the even / odd maxima; full=False removes cal_remove_dim(dims) >= 0 columns and takes the maximum over groups of dims columns.

    return_route=True: -> (out, route), route [B, dims] int16, not differentiable: for full=False the first group that attains the column's
    maximum; for full=True 2 * g + s with s = 0 where pos > neg and 1 otherwise, g the first group that attains the maximum of the chosen
    column (2j for s = 0, 2j + 1 for s = 1).  A winner may lie in the zero padding.  The backward writes the whole [B, V] gradient row in one
    pass: +grad (s = 0) or -grad (s = 1) at the routed column, zero everywhere else, nothing for a winner in the padding.

    aggregate works row by row, so aggregating each device's reps before the cross-device gather (modeling.py:160-164) gives the same scores
    as the reference's order, gather first, and gathers [B, dims] instead of [B, V].

    ValueError / RuntimeError as `dhr_amd.lexical.aggregate` raises them (rank; a negative remove with full=False; a vocabulary that does
    not split into whole groups), DhrError for dtypes, devices, no GPU or more than 16383 groups."""
    dims, full = int(dims), bool(full)
    _check_aggregate(lexical_reps, dims, full)
    out, route = _functions()[0].apply(lexical_reps, dims, full)
    return (out, route) if return_route else out


def term_weight_reps(input_ids, term_weights, vocab: int = VOCAB_SIZE, skip_tokens: int = 1, return_tokens: bool = False):
    """The lexical reps of the head without the MLM logits (--skip_mlm, modeling.py:279-284, 311-316) with `.backward()` to `term_weights`:

        reps[b][v] = max(0, max over {t : input_ids[b][skip_tokens + t] == v} of term_weights[b][t])        -> [B, vocab] fp32

    which is what the reference's scatter into a zero [B, L, vocab] tensor followed by the max over tokens yields, its zero tensor always
    holding an untouched row.  `input_ids` [B, L] int32 or int64 are the model's whole ids, the first skip_tokens take no part;
    `term_weights` is [B, L - skip_tokens] or [B, L - skip_tokens, 1], fp16 or fp32 (fp16 weights are widened exactly); at most 32767 tokens.

    There is no attention mask, as in the reference: a padding token deposits its weight at its own id (0 for [PAD]), where it competes like
    any other token.  Ids outside [0, vocab) are ignored (the reference raises or device-asserts).  When an id repeats within a row the
    largest weight wins and, among equal weights, the first position, whatever the execution order: two runs are bit-identical.

    return_tokens=True: -> (reps, tok), tok [B, vocab] int16, not differentiable: the first token (counted after the skipped ones) that
    attains a strictly positive maximum, -1 where the zero wins.  The backward is the gather dw[b][t] = grad[b][v] where tok[b][v] == t
    (v = input_ids[b][skip_tokens + t]), else 0, in the weights' dtype and shape.

    One deviation from the reference: a weight of exactly 0.0 never takes the gradient here (the zero wins).  The reference's first-index
    rule would hand it the gradient only where every earlier row of its [B, L, vocab] tensor held the same id, i.e. for the first tokens of a
    row when they all carry that id.

    ValueError for wrong ranks / shapes or no tokens, DhrError for dtypes, devices or no GPU."""
    vocab, skip_tokens = int(vocab), int(skip_tokens)
    _check_term_weights(input_ids, term_weights, vocab, skip_tokens)
    reps, tok = _functions()[1].apply(input_ids, term_weights, vocab, skip_tokens)
    return (reps, tok) if return_tokens else reps
