"""The lexical head of the DHR / Aggretriever encoders for TRAINING with the vocabulary projection fused in: differentiable, on the HIP ops
`dhr_lexical_proj_train` and `dhr_lexical_proj_backward` (dhr_amd/csrc/lexical_proj_train.hip).

`dhr_amd.lexical_train` starts from the MLM logits [B, L, V] and returns their gradient: two B * L * V tensors of a training step.  This
module starts one GEMM earlier, from the input of the vocabulary projector, its weight and its bias, as `dhr_amd.lexical_proj` does for
encoding:

    lexical_reps(hidden, weight, bias, term_weights, attention_mask, skip_tokens=0, return_tokens=False)   -> [B, V] fp32 reps (or (reps, tok))

and `.backward()` returns the gradients of `hidden`, `weight`, `bias` and `term_weights`.  The logits and their gradient exist only in
registers and LDS; besides its inputs the op keeps the reps, the int16 token that attains each maximum, the softmax value of that token
(fp32 [B, V]) and under 256 bytes per token.  Masked tokens are never multiplied.  The forward values are bit-identical to
`dhr_amd.lexical_proj.lexical_reps` on the same fp16 or bf16 operands.

Arguments: `hidden` [B, L, H], the input of the vocabulary projector (DistilBERT: the output of `vocab_layer_norm`), and `weight` [V, H]: fp16,
bf16 or fp32.  The kernels read both in one 16-bit type: bf16 if either is bf16, else fp16 (one fp16 and one bf16 is a DhrError); an fp32
operand is rounded to that type once, as autocast's `linear` does with the fp32 states of a layer norm and an fp32 master weight.  H is a
multiple of 8, at most 1024.  `bias` [V] fp16 / bf16 / fp32 or None.  `skip_tokens = s` drops the first s tokens; `term_weights` ([B, L - s] or
[B, L - s, 1], a floating dtype) and `attention_mask` ([B, L - s] or [B, L - s, 1]) are what the reference slices with [:, 1:].  Pass the
model's whole hidden states with skip_tokens=1, or the `[:, 1:]` view with skip_tokens=0: the same bits.  fp16 and bf16 tensors are read in place
whatever their batch / token / row strides, the last dimension contiguous.

Gradients: to `hidden` (all L tokens; skipped and masked rows are exact zeros), `weight` (a plain [V, H] tensor, so tied word embeddings
accumulate it through autograd), `bias` and `term_weights` (in its shape), each in its input's dtype, rounded once from fp32 accumulators;
only those that `needs_input_grad` lists are computed (a frozen projector runs no weight-gradient pass, a detached `hidden` no
hidden-gradient pass).  `attention_mask` and `tok` are not differentiable.  At a tie the first token takes the gradient, like torch.max.
Every sum runs in a fixed order without atomics: two runs on the same inputs are bit-identical.  Everything is enqueued on torch's current
stream of `hidden`'s device, without a host synchronisation; buffers come from torch's allocator.  The backward takes every address from the
tensors that autograd hands back, so saved-tensor hooks (`save_on_cpu`, non-reentrant checkpointing) work.  There is no CPU implementation."""
from __future__ import annotations

from . import _lexical_args as A
from . import _lib
from . import _marshal as M

MAX_TOKENS = 32767
MAX_HIDDEN = 1024


def _check(hidden, weight, bias, term_weights, attention_mask, skip_tokens):
    """Shape / dtype / device checks, before the library is touched.  -> (B, L, T, H, V)"""
    import torch
    for a in (hidden, weight, term_weights, attention_mask) + (() if bias is None else (bias,)):
        if not isinstance(a, torch.Tensor):
            raise _lib.DhrError("lexical_proj_train.lexical_reps: torch tensors on a GPU are required (there is no host path)")
    if hidden.dim() != 3:
        raise ValueError('hidden must be [batch, tokens, hidden size], got {} dimensions'.format(hidden.dim()))
    B, L, H = (int(d) for d in hidden.shape)
    if weight.dim() != 2 or int(weight.shape[1]) != H:
        raise ValueError('weight must be [vocab, hidden size {}], got {}'.format(H, tuple(weight.shape)))
    V = int(weight.shape[0])
    if V == 0 or H == 0:
        raise ValueError('weight has no rows or no columns')
    if bias is not None and (bias.dim() != 1 or int(bias.shape[0]) != V):
        raise ValueError("bias does not match the vocabulary")
    T = A.check_token_side(term_weights, attention_mask, B, L, skip_tokens, MAX_TOKENS)
    ok = (torch.float16, torch.bfloat16, torch.float32)
    if hidden.dtype not in ok or weight.dtype not in ok:
        raise _lib.DhrError(f"unsupported hidden / weight dtype {hidden.dtype} / {weight.dtype} (float16 / bfloat16 / float32)")
    if {hidden.dtype, weight.dtype} == {torch.float16, torch.bfloat16}:
        raise _lib.DhrError(f"hidden / weight dtype {hidden.dtype} / {weight.dtype}: one float16 and one bfloat16 operand have no common 16-bit type")
    if bias is not None and bias.dtype not in ok:
        raise _lib.DhrError(f"unsupported bias dtype {bias.dtype} (float16 / bfloat16 / float32)")
    if H % 8 or H > MAX_HIDDEN:
        raise _lib.DhrError(f"lexical_proj_train.lexical_reps: the hidden size {H} is not a multiple of 8 up to {MAX_HIDDEN}")
    if not hidden.is_cuda:
        raise _lib.DhrError("lexical_proj_train.lexical_reps: hidden must live on a GPU (there is no CPU implementation)")
    for a in (weight, term_weights, attention_mask) + (() if bias is None else (bias,)):
        if a.device != hidden.device:
            raise _lib.DhrError("lexical_proj_train.lexical_reps: hidden, weight, bias, term_weights and attention_mask must live on one device")
    return B, L, T, H, V


def _operand_dtype(hidden, weight):
    """the 16-bit type the kernels read both operands in: bfloat16 if either is, else float16"""
    return "bfloat16" if "bfloat16" in (M.dtype_name(hidden), M.dtype_name(weight)) else "float16"


def _rows16(a, dtype):
    """the 16-bit operand as the kernels read it: rounded once if fp32, the last dimension contiguous, rows (and batches) not overlapping"""
    return M.as_read(M.cast(a.detach(), dtype))[0]


def _head_args(h, W, b, w, m, B, T, skip_tokens, H, V):
    """the arguments that dhr_lexical_proj_train and dhr_lexical_proj_backward share, from the tensors as they are NOW
    (h, W: as _rows16 returns them, of one dtype; b, w [B, T], m [B, T]: contiguous)"""
    return (M.device(h), _lib.MEM_DEVICE, h.data_ptr(), _lib._val_code(h, bf16=True), B, T, skip_tokens, H, *M.lds(h), W.data_ptr(), V, *M.lds(W), M.data_ptr(b),
            _lib.VAL_F32 if b is None else _lib._val_code(b, bf16=True), w.data_ptr(), T, m.data_ptr(), T)


def _function():
    """The torch.autograd.Function (built on first use, like dhr_amd.lexical_train)."""
    global _FN
    if _FN is not None:
        return _FN
    import torch

    class LexicalProjReps(torch.autograd.Function):
        @staticmethod
        def forward(ctx, hidden, weight, bias, term_weights, attention_mask, skip_tokens):
            B, L, T, H, V = _check(hidden, weight, bias, term_weights, attention_mask, skip_tokens)
            lib = _lib.load()
            dev = hidden.device
            op = _operand_dtype(hidden, weight)
            h, W = _rows16(hidden, op), _rows16(weight, op)
            b = A.bias_as_read(bias, op, dev)
            w, m = A.tokens_f32(term_weights, B, T), A.tokens_f32(attention_mask, B, T)
            reps = torch.empty((B, V), dtype=torch.float32, device=dev)
            tok = torch.empty((B, V), dtype=torch.int16, device=dev)
            pwin = torch.empty((B, V), dtype=torch.float32, device=dev)
            n_ws = int(lib.dhr_lexical_proj_train_workspace(B, T, V, H)) if B else 0
            ws = torch.empty((max(n_ws, 16),), dtype=torch.uint8, device=dev)
            if B:
                _lib.check(lib.dhr_lexical_proj_train(*_head_args(h, W, b, w, m, B, T, skip_tokens, H, V), reps.data_ptr(), V, tok.data_ptr(), V,
                                                      pwin.data_ptr(), V, ws.data_ptr(), n_ws, M.stream(h)), "dhr_lexical_proj_train")
            ctx.save_for_backward(h, W, b, w, m, tok, pwin, ws)
            ctx.geom = (B, L, T, H, V, skip_tokens, n_ws, hidden.dtype, weight.dtype, None if bias is None else bias.dtype,
                        tuple(term_weights.shape), term_weights.dtype)
            ctx.mark_non_differentiable(tok)
            return reps, tok

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad, _grad_tok):
            # ctx keeps scalars only: saved-tensor hooks (save_on_cpu, checkpointing) may hand back the tensors at other addresses
            h, W, b, w, m, tok, pwin, ws = ctx.saved_tensors
            h, W = _rows16(h, h.dtype), _rows16(W, W.dtype)     # (no copies unless a hook changed the layout)
            b, w, m, tok, pwin, ws = (None if t is None else t.contiguous() for t in (b, w, m, tok, pwin, ws))
            B, L, T, H, V, skip_tokens, n_ws, h_dtype, W_dtype, b_dtype, w_shape, w_dtype = ctx.geom
            need_h, need_W, need_b, need_w = ctx.needs_input_grad[:4]
            need_b = need_b and b is not None
            if not (need_h or need_W or need_b or need_w):
                return None, None, None, None, None, None
            lib = _lib.load()
            dev = h.device
            g, ld_g = M.grad_rows(grad, B, V)
            dh = torch.empty((B, L, H), dtype=h_dtype, device=dev) if need_h else None
            dW = torch.empty((V, H), dtype=W_dtype, device=dev) if need_W else None
            db = torch.empty((V,), dtype=b.dtype, device=dev) if need_b else None     # (fp32 where the forward widened the bias)
            dw = torch.empty((B, T), dtype=torch.float32, device=dev) if need_w else None
            if B:
                ptr, code = M.data_ptr, lambda t: _lib.VAL_F32 if t is None else _lib._val_code(t, bf16=True)
                _lib.check(lib.dhr_lexical_proj_backward(*_head_args(h, W, b, w, m, B, T, skip_tokens, H, V), g.data_ptr(), ld_g,
                                                         tok.data_ptr(), V, pwin.data_ptr(), V, ws.data_ptr(), n_ws, ptr(dh), code(dh), L * H, H,
                                                         ptr(dW), code(dW), H, ptr(db), code(db), ptr(dw), T, M.stream(h)),
                           "dhr_lexical_proj_backward")
            else:
                for t in (dW, db):
                    if t is not None:
                        t.zero_()
            return dh, dW, (None if db is None else db.to(b_dtype)), (None if dw is None else dw.to(w_dtype).reshape(w_shape)), None, None

    _FN = LexicalProjReps
    return _FN


_FN = None


def lexical_reps(hidden, weight, bias, term_weights, attention_mask, skip_tokens: int = 0, return_tokens: bool = False):
    """-> [B, V] fp32 lexical reps, torch.max((softmax(hidden[:, skip_tokens:] @ weight.T + bias) * term_weights) * attention_mask,
    dim=-2).values, with `.backward()` to `hidden`, `weight`, `bias` and `term_weights`.  return_tokens=True: -> (reps, tok), tok [B, V] int16
    the first token (counted after the skipped ones) that attains each maximum.  ValueError for wrong ranks / shapes or no tokens, DhrError
    for dtypes, devices or no GPU."""
    skip_tokens = int(skip_tokens)
    _check(hidden, weight, bias, term_weights, attention_mask, skip_tokens)
    reps, tok = _function().apply(hidden, weight, bias, term_weights, attention_mask, skip_tokens)
    return (reps, tok) if return_tokens else reps
