"""What the four lexical-head modules (lexical, lexical_proj, lexical_train, lexical_proj_train) do alike with their arguments, once: the
token-side operands as fp32 [B, T], the check of the token-side arguments of the training modules, the projection's bias as the kernels read
it, and the output record of the encoding modules as the arguments of the C ABI."""
from __future__ import annotations

import numpy as np

from . import _lib
from . import _marshal as M


def tokens_f32(a, B, T, like=None):
    """term_weights / attention_mask -> detached fp32 [B, T], contiguous.  like: a numpy array -> numpy; a tensor -> on its device; None -> a
    tensor where `a` lives (the training modules, which refuse operands on different devices before they get here)."""
    if like is not None and M.is_np(like):
        return np.ascontiguousarray(np.asarray(a).reshape(B, T), dtype=np.float32)
    import torch
    a = a.detach().reshape(B, T)
    return (a.to(torch.float32) if like is None else a.to(device=like.device, dtype=torch.float32)).contiguous()


def check_token_side(term_weights, attention_mask, B, L, skip_tokens, max_tokens):
    """The token-side rules of the training modules -> T, the tokens after the skipped ones."""
    if skip_tokens < 0:
        raise ValueError('skip_tokens must be >= 0, got {}'.format(skip_tokens))
    T = L - skip_tokens
    if T <= 0:
        raise ValueError('no tokens: the maximum over tokens of an empty sequence is undefined ({} tokens, {} skipped)'.format(L, skip_tokens))
    for a, what in ((term_weights, "term_weights"), (attention_mask, "attention_mask")):
        if tuple(a.shape) not in ((B, T), (B, T, 1)):
            raise ValueError('{} must be [{}, {}] or [{}, {}, 1] (batch, tokens - skip_tokens), got {}'.format(what, B, T, B, T, tuple(a.shape)))
    if T > max_tokens:
        raise ValueError('more than {} tokens'.format(max_tokens))
    if not term_weights.dtype.is_floating_point:
        raise _lib.DhrError(f"unsupported term_weights dtype {term_weights.dtype} (a floating-point dtype)")
    return T


def bias_as_read(bias, operand_dtype, device):
    """The projection's bias [V] as the kernels read it, None for none: detached, on `device`, contiguous; a bf16 bias next to fp16 operands is
    widened to fp32 (the fp16 kernels read fp32 or fp16: [V] values, widened exactly)."""
    if bias is None:
        return None
    b = bias.detach().to(device).contiguous()
    return b.float() if M.dtype_name(b) == "bfloat16" and M.dtype_name(operand_dtype) == "float16" else b


def record_outputs(value_out, index_out, semantic_reps, batch, kind, wrong_kind):
    """The output record of an encoding call -> ((value pointer, ld), (index pointer, dtype code, ld, cls pointer, dtype code, ld, cls_dim),
    keepalive), the last seven in the order of the C ABI.  Every array must live in memory kind `kind`, else wrong_kind(name) is raised;
    semantic_reps [batch, cls_dim] of another dtype than fp16 / fp32 are converted (the keepalive)."""
    def in_kind(name, a):
        if (_lib.MEM_DEVICE if getattr(a, "is_cuda", False) else _lib.MEM_HOST) != kind:
            raise wrong_kind(name)
        return a
    value = _lib._ptr_ld(in_kind("value_out", value_out))[:2]
    index, cls, c = (None, _lib.IDX_NONE, 0), (None, _lib.VAL_F16, 0, 0), None
    if index_out is not None:
        p_i, ld_i, _ = _lib._ptr_ld(in_kind("index_out", index_out))
        index = (p_i, _lib.idx_code(index_out.dtype), ld_i)
    if semantic_reps is not None:
        c = in_kind("semantic_reps", semantic_reps)
        c = M.values(c if M.is_np(c) else c.detach())
        p_c, ld_c, _ = _lib._ptr_ld(c)
        if int(c.shape[0]) != batch:
            raise ValueError("semantic reps do not match the batch")
        cls = (p_c, _lib._val_code(c), ld_c, int(c.shape[1]))
    return value, index + cls, c
