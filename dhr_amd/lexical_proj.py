"""The lexical head of an encoding run with the vocabulary projection fused in, on the HIP op `dhr_lexical_proj_head`.

`dhr_amd.lexical` starts from the MLM logits [B, T, V], which the model writes with the last linear layer of its MLM head (H -> V).  This
module starts one GEMM earlier: from that layer's input, its weight and its bias.  The logits are never written to memory and masked tokens
are never multiplied:

    lexical_reps(hidden, weight, bias, term_weights, attention_mask)                          -> [B, V] fp32 reps
    densify_lexical_into(..., value_out, index_out, dims, remove_dims, semantic_reps)          DHR / DLR records
    aggregate_lexical_into(..., value_out, agg_dim, full, semantic_reps)                       Aggretriever records

Arguments: `hidden` [B, T, H] fp16 or bf16, the input of the vocabulary projector (DistilBERT: the output of `vocab_layer_norm`; BERT: of
`cls.predictions.transform`); pass the `[:, 1:]` view: any batch / token strides, the last dimension contiguous, H a multiple of 8, read in
place.  `weight` [V, H] of the same dtype as `hidden` (any row stride), `bias` [V] fp16 / bf16 / fp32 or None (a bf16 bias next to
fp16 operands is widened to fp32 first, exactly).  `term_weights`, `attention_mask`, the outputs and what is written into them are those of
`dhr_amd.lexical`; the logits are x = hidden @ weight.T + bias with fp32 products and sums (of the bf16 values where the operands are bf16:
their range is kept) and are not rounded to 16 bits.

Torch CUDA tensors only: the op runs on their device, enqueues on the current stream and does not wait.  CPU tensors and numpy arrays raise
DhrError: there is no staged host path and no CPU implementation."""
from __future__ import annotations

from . import _lexical_args as A
from . import _lib
from . import _marshal as M
from .lexical import _agg_geometry, _check_out, _densify_check


def _not_on_gpu(name):
    return _lib.DhrError(f"lexical projection head: {name} must be a torch tensor on the GPU (there is no host path)")


def _on_gpu(name, a):
    if not getattr(a, "is_cuda", False):
        raise _not_on_gpu(name)


def _run(mode, hidden, weight, bias, term_weights, attention_mask, value_out, index_out, dims, remove_dims, semantic_reps):
    import torch
    for name, a in (("hidden", hidden), ("weight", weight), ("value_out", value_out)):
        _on_gpu(name, a)
    if hidden.dim() != 3:
        raise ValueError('hidden must be [batch, tokens, hidden size], got {} dimensions'.format(hidden.dim()))
    if weight.dim() != 2 or int(weight.shape[1]) != int(hidden.shape[2]):
        raise ValueError('weight must be [vocab, hidden size {}], got {}'.format(int(hidden.shape[2]), tuple(weight.shape)))
    B, T, H = (int(d) for d in hidden.shape)
    V = int(weight.shape[0])
    if T == 0:
        raise ValueError('no tokens: the maximum over tokens of an empty sequence is undefined')
    if hidden.dtype not in (torch.float16, torch.bfloat16) or weight.dtype != hidden.dtype:
        raise _lib.DhrError(f"unsupported hidden / weight dtype {hidden.dtype} / {weight.dtype} (both float16 or both bfloat16)")
    if H % 8:
        raise _lib.DhrError(f"lexical projection head: the hidden size {H} is not a multiple of 8")
    lib = _lib.load()
    dev = hidden.device
    hidden, (ld_batch, ld_token) = M.as_read(hidden.detach())
    if weight.device != dev:
        raise _lib.DhrError("lexical projection head: hidden and weight must live on the same GPU")
    weight, (ld_weight,) = M.as_read(weight.detach())
    if bias is not None:
        _on_gpu("bias", bias)
        if bias.dtype not in (torch.float16, torch.bfloat16, torch.float32):
            raise _lib.DhrError(f"unsupported bias dtype {bias.dtype} (float16 / bfloat16 / float32)")
        if bias.dim() != 1 or int(bias.shape[0]) != V:
            raise ValueError("bias does not match the vocabulary")
    bias = A.bias_as_read(bias, hidden.dtype, dev)
    b_dt = _lib.VAL_F32 if bias is None else _lib._val_code(bias, bf16=True)
    w, m = A.tokens_f32(term_weights, B, T, hidden), A.tokens_f32(attention_mask, B, T, hidden)
    (p_v, ld_v), record, _keep = A.record_outputs(value_out, index_out, semantic_reps, B, _lib.MEM_DEVICE, _not_on_gpu)  # (_keep: converted semantic reps)
    if B:
        n_ws = int(lib.dhr_lexical_proj_workspace(B, T, V, mode))
        ws = torch.empty(max(n_ws, 16), dtype=torch.uint8, device=dev)
        _lib.check(lib.dhr_lexical_proj_head(M.device(hidden), _lib.MEM_DEVICE, mode, hidden.data_ptr(), _lib._val_code(hidden, bf16=True), B, T, H, ld_batch, ld_token,
                                             weight.data_ptr(), V, ld_weight, M.data_ptr(bias), b_dt, w.data_ptr(), T, m.data_ptr(), T, dims, remove_dims, p_v,
                                             _lib._val_code(value_out), ld_v, *record, ws.data_ptr(), n_ws, M.stream(hidden)), "dhr_lexical_proj_head")
        # (the call is asynchronous; the temporaries were allocated on the stream it runs on, so the allocator reuses them only behind it)
    return B, V


def lexical_reps(hidden, weight, bias, term_weights, attention_mask):
    """-> [B, V] fp32 lexical reps, torch.max((softmax(hidden @ weight.T + bias) * term_weights) * attention_mask, dim=-2).values."""
    import torch
    _on_gpu("hidden", hidden)
    out = torch.empty((int(hidden.shape[0]), int(weight.shape[0])), dtype=torch.float32, device=hidden.device)
    _run(_lib.LEX_RAW, hidden, weight, bias, term_weights, attention_mask, out, None, 0, 0, None)
    return out


def densify_lexical_into(hidden, weight, bias, term_weights, attention_mask, value_out, index_out, dims: int = 768, remove_dims: int = 570,
                         semantic_reps=None):
    """`dhr_amd.lexical.densify_lexical_into` from the projector's input: the densified reps into the first `dims` columns of the record's
    value array (fp16 or fp32) and its index array (uint8, or int16 beyond 256 groups), semantic_reps [B, cls_dim] into the value columns
    that follow.  -> (value_out, index_out)."""
    B, V = int(hidden.shape[0]), int(weight.shape[0])
    _densify_check(V, dims, remove_dims)
    cls = 0 if semantic_reps is None else int(semantic_reps.shape[1])
    _check_out(value_out, B, dims + cls)
    _check_out(index_out, B, dims)
    _run(_lib.LEX_DENSIFY, hidden, weight, bias, term_weights, attention_mask, value_out, index_out, dims, remove_dims, semantic_reps)
    return value_out, index_out


def aggregate_lexical_into(hidden, weight, bias, term_weights, attention_mask, value_out, agg_dim: int = 640, full: bool = True,
                           semantic_reps=None):
    """`dhr_amd.lexical.aggregate_lexical_into` from the projector's input: aggregate(reps, agg_dim, full) (+ merge_reps with
    semantic_reps) into the record's value array [B, >= agg_dim + cls_dim] (fp16 or fp32).  -> value_out."""
    B, V = int(hidden.shape[0]), int(weight.shape[0])
    remove, _ = _agg_geometry(B, V, agg_dim, full)
    cls = 0 if semantic_reps is None else int(semantic_reps.shape[1])
    _check_out(value_out, B, agg_dim + cls)
    _run(_lib.LEX_AGG_FULL if full else _lib.LEX_AGG_SEMI, hidden, weight, bias, term_weights, attention_mask, value_out, None, agg_dim, remove,
         semantic_reps)
    return value_out
