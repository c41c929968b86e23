"""The lexical head of the DHR / Aggretriever encoders for TRAINING: differentiable, on the HIP ops `dhr_lexical_head_train` and
`dhr_lexical_head_backward` (dhr_amd/csrc/lexical_train.hip).

The reference computes, in eager torch with autograd on (tevatron/DHR/modeling.py:294-300, 325-331, tevatron/Aggretriever/modeling.py:274-278,
306-310),

    p_logits = softmax(psg_out.logits[:, 1:])                                                  # fp32 [B, L-1, V], kept by autograd
    p_lexical_reps = torch.max((p_logits * p_term_weights) * attention_mask, dim=-2).values    # two more fp32 [B, L-1, V] + int64 [B, V]

Here

    lexical_reps(logits, term_weights, attention_mask, skip_tokens=0, return_tokens=False)     -> [B, V] fp32 reps  (or (reps, tok))

keeps, besides its inputs, the reps, the int16 token that attains each maximum and 20 bytes per token; `.backward()` recomputes the softmax
from the logits and writes the gradient of the logits in one streaming pass.  The forward values are bit-identical to
`dhr_amd.lexical.lexical_reps` (which detaches its inputs and serves encoding).

Arguments: `logits` [B, L, V] fp16, bf16 or fp32 on a GPU (any batch / token strides, the last dimension contiguous); `skip_tokens = s` drops the
first s tokens, so `term_weights` ([B, L - s] or [B, L - s, 1], fp16 / fp32) and `attention_mask` ([B, L - s] or [B, L - s, 1], any integer,
bool or float dtype) are what the reference slices with [:, 1:].  Pass the model's whole logits with skip_tokens=1: the gradient of the
whole tensor is then written in one pass (rows of skipped and masked tokens as zeros), where autograd's backward of a `[:, 1:]` view would
add a memset and a copy of the largest tensor of the step.  The view with skip_tokens=0 works too and gives the same numbers.

Differentiable with respect to `logits` (the gradient comes back in their dtype, fp16 / bf16 rounded once from fp32) and `term_weights` (in their dtype and shape);
`attention_mask` and `tok` are not differentiable.  At a tie the first token takes the gradient, like torch.max.  The sums of the backward
run in a fixed order: two runs on the same inputs are bit-identical.  Everything is enqueued on torch's current stream of the logits'
device, without a host synchronisation; buffers come from torch's allocator.  There is no CPU implementation: without a GPU the call raises."""
from __future__ import annotations

from . import _lexical_args as A
from . import _lib
from . import _marshal as M

MAX_TOKENS = 32767


def _check(logits, term_weights, attention_mask, skip_tokens):
    """Shape / dtype / device checks, before the library is touched.  -> (B, L, T, V)"""
    import torch
    if not isinstance(logits, torch.Tensor) or not isinstance(term_weights, torch.Tensor) or not isinstance(attention_mask, torch.Tensor):
        raise _lib.DhrError("lexical_train.lexical_reps: torch tensors on a GPU are required (dhr_amd.lexical serves numpy arrays, without gradients)")
    if logits.dim() != 3:
        raise ValueError('logits must be [batch, tokens, vocab], got {} dimensions'.format(logits.dim()))
    B, L, V = (int(d) for d in logits.shape)
    if V == 0:
        raise ValueError('logits have no vocabulary columns')
    T = A.check_token_side(term_weights, attention_mask, B, L, skip_tokens, MAX_TOKENS)
    if logits.dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise _lib.DhrError(f"unsupported logits dtype {logits.dtype} (float16 / bfloat16 / float32)")
    if not logits.is_cuda:
        raise _lib.DhrError("lexical_train.lexical_reps: the logits must live on a GPU (there is no CPU implementation)")
    if term_weights.device != logits.device or attention_mask.device != logits.device:
        raise _lib.DhrError("lexical_train.lexical_reps: logits, term_weights and attention_mask must live on one device")
    return B, L, T, V


def _function():
    """The torch.autograd.Function (built on first use, like dhr_amd.gip_scores)."""
    global _FN
    if _FN is not None:
        return _FN
    import torch

    class LexicalReps(torch.autograd.Function):
        @staticmethod
        def forward(ctx, logits, term_weights, attention_mask, skip_tokens):
            B, L, T, V = _check(logits, term_weights, attention_mask, skip_tokens)
            lib = _lib.load()
            x, (ld_batch, ld_token) = M.as_read(logits.detach())
            w, m = A.tokens_f32(term_weights, B, T), A.tokens_f32(attention_mask, B, T)
            reps = torch.empty((B, V), dtype=torch.float32, device=x.device)
            tok = torch.empty((B, V), dtype=torch.int16, device=x.device)
            ws = torch.empty((int(lib.dhr_lexical_head_train_workspace(B, T)) if B else 0,), dtype=torch.uint8, device=x.device)
            if B:
                _lib.check(lib.dhr_lexical_head_train(M.device(x), _lib.MEM_DEVICE, x.data_ptr(), _lib._val_code(x, bf16=True), B, T, skip_tokens, V, ld_batch,
                                                      ld_token, w.data_ptr(), T, m.data_ptr(), T, reps.data_ptr(), V, tok.data_ptr(), V, ws.data_ptr(),
                                                      M.stream(x)), "dhr_lexical_head_train")
            ctx.save_for_backward(x, tok, ws)
            ctx.geom = (B, L, T, V, skip_tokens, tuple(term_weights.shape), term_weights.dtype)
            ctx.mark_non_differentiable(tok)
            return reps, tok

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad, _grad_tok):
            x, tok, ws = ctx.saved_tensors
            B, L, T, V, skip_tokens, w_shape, w_dtype = ctx.geom
            need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
            if not (need_x or need_w):
                return None, None, None, None
            lib = _lib.load()
            g, ld_g = M.grad_rows(grad, B, V)
            ld_batch, ld_token = M.lds(x)
            dx = torch.empty((B, L, V), dtype=x.dtype, device=x.device) if need_x else None
            dw = torch.empty((B, T), dtype=torch.float32, device=x.device) if need_w else None
            if B:
                _lib.check(lib.dhr_lexical_head_backward(M.device(x), _lib.MEM_DEVICE, x.data_ptr(), _lib._val_code(x, bf16=True), B, T, skip_tokens, V, ld_batch,
                                                         ld_token, g.data_ptr(), ld_g, tok.data_ptr(), V, ws.data_ptr(), M.data_ptr(dx), L * V, V,
                                                         M.data_ptr(dw), T, M.stream(x)), "dhr_lexical_head_backward")
            return dx, (None if dw is None else dw.to(w_dtype).reshape(w_shape)), None, None

    _FN = LexicalReps
    return _FN


_FN = None


def lexical_reps(logits, term_weights, attention_mask, skip_tokens: int = 0, return_tokens: bool = False):
    """-> [B, V] fp32 lexical reps, torch.max((softmax(logits[:, skip_tokens:]) * term_weights) * attention_mask, dim=-2).values, with
    `.backward()` to `logits` and `term_weights`.  return_tokens=True: -> (reps, tok), tok [B, V] int16 the first token (counted after the
    skipped ones) that attains each maximum.  ValueError for wrong ranks / shapes or no tokens, DhrError for dtypes, devices or no GPU."""
    skip_tokens = int(skip_tokens)
    _check(logits, term_weights, attention_mask, skip_tokens)
    reps, tok = _function().apply(logits, term_weights, attention_mask, skip_tokens)
    return (reps, tok) if return_tokens else reps
