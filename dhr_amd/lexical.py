"""The lexical head of the DHR / Aggretriever encoders on the fused HIP op `dhr_lexical_head`, and the Aggretriever twin of
`dhr_amd.densify.densify` (`aggregate`, `cal_remove_dim`, tevatron/Aggretriever/utils.py) on the same kernel.

The reference computes, in eager torch (tevatron/DHR/modeling.py:297-300, tevatron/Aggretriever/modeling.py:274-278),

    p_logits = softmax(psg_out.logits[:, 1:])                                                  # fp32 [B, L-1, V]
    p_lexical_reps = torch.max((p_logits * p_term_weights) * attention_mask, dim=-2).values    # [B, V]

and the encoder driver then densifies (DHR) or aggregates (Aggretriever) the reps and casts them to fp16 into the index record
(tevatron/driver/encode.py:149-194).  Here one op reads the logits and writes the record:

    lexical_reps(logits, term_weights, attention_mask)                          -> [B, V] fp32 reps
    densify_lexical_into(..., value_out, index_out, dims, remove_dims, semantic_reps)   DHR / DLR records
    aggregate_lexical_into(..., value_out, agg_dim, full, semantic_reps)                Aggretriever records

Arguments: `logits` [B, T, V] fp16, bf16 (torch tensors on a GPU; numpy has no bf16) or fp32 (pass `psg_out.logits[:, 1:]`: any batch /
token strides, the last dimension contiguous, the view is read in place), `term_weights` [B, T] or [B, T, 1] fp16 / fp32, `attention_mask`
[B, T] or [B, T, 1] of any integer or bool dtype (the reference's `psg['attention_mask'][:, 1:]`).  16-bit logits widen to fp32 exactly, so
the same values in fp16 and in bf16 give the same bits.  Each contribution is (p * w) * mask in fp32, so a masked token folds in a zero with
the sign of its weight, and ties keep the first token and the first group, like torch.max on the device.  Finite logits and -inf are in
scope; NaN and +inf are not, and every unmasked token needs one finite logit.

Torch CUDA tensors are processed on their device and on torch's current stream; the calls wait for that stream, so the outputs are complete
on return.  numpy arrays are staged through device 0.  There is no CPU implementation: without the HIP library / a GPU the calls raise."""
from __future__ import annotations

import numpy as np

from . import _lexical_args as A
from . import _lib
from . import _marshal as M

VOCAB_SIZE = 30522


def cal_remove_dim(dims, vocab_size=VOCAB_SIZE):
    """tevatron/Aggretriever/utils.py:8-14: the unused leading vocabulary ids (negative: zero columns padded at the end)."""
    remove_dims = vocab_size % dims
    if remove_dims > 1000:  # the first 1000 tokens in BERT are useless
        remove_dims -= dims
    return remove_dims


def _agg_geometry(batch, vocab, dims, full):
    """-> (remove, group width) of aggregate(), raising what the reference's view raises."""
    if full:
        remove, width = cal_remove_dim(dims * 2), dims * 2
        cols = vocab - remove if remove < 0 else max(0, vocab - remove)
    else:
        remove, width = cal_remove_dim(dims), dims
        if remove < 0:
            raise ValueError('aggregate(full=False): cal_remove_dim({}) = {} is negative; the semi-aggregated view does not exist'.format(dims, remove))
        cols = max(0, vocab - remove)
    if batch * cols == 0:
        raise RuntimeError("cannot reshape tensor of 0 elements into shape [{}, -1, {}] because the unspecified dimension size -1 can be any "
                           "value and is ambiguous".format(batch, width))
    if cols % width:
        raise RuntimeError("shape '[{}, -1, {}]' is invalid for input of size {}".format(batch, width, batch * cols))
    return remove, width


def _densify_check(vocab, dims, remove_dims):
    if (vocab - remove_dims) % dims != 0:                                                    # tevatron/DHR/utils.py:14-16
        raise ValueError('Input lexical representation cannot be densified, please fix dims or remove_dims')


def _inputs(logits, term_weights, attention_mask):
    """-> (logits view, batch / token strides, w fp32 [B, T], mask fp32 [B, T], B, T, V)."""
    if len(logits.shape) != 3:
        raise ValueError('logits must be [batch, tokens, vocab], got {} dimensions'.format(len(logits.shape)))
    B, T, V = (int(d) for d in logits.shape)
    if T == 0:
        raise ValueError('no tokens: the maximum over tokens of an empty sequence is undefined')
    if M.dtype_name(logits) not in M.FLOATS + ("bfloat16",):
        raise _lib.DhrError(f"unsupported logits dtype {logits.dtype} (float16 / bfloat16 / float32)")
    if M.dtype_name(logits) == "bfloat16" and (M.is_np(logits) or not logits.is_cuda):
        raise _lib.DhrError("lexical head: bfloat16 logits must live on a GPU (the staged host path serves numpy arrays, which have no bfloat16)")
    w, m = A.tokens_f32(term_weights, B, T, logits), A.tokens_f32(attention_mask, B, T, logits)
    if not M.is_np(logits):
        logits = logits.detach()
    logits, (ldb, ldt) = M.as_read(logits)
    return logits, ldb, ldt, w, m, B, T, V


def _wrong_kind(name):
    return _lib.DhrError("lexical head: semantic reps must live in the same memory kind as the logits" if name == "semantic_reps" else
                         "lexical head: inputs and outputs must live in the same memory kind")


def _run(mode, logits, term_weights, attention_mask, value_out, index_out, dims, remove_dims, semantic_reps):
    lg, ldb, ldt, w, m, B, T, V = _inputs(logits, term_weights, attention_mask)     # (its dtype checks come before the library is touched)
    lib = _lib.load()
    kind = M.mem_kind(lg)
    (p_v, ld_v), record, _keep = A.record_outputs(value_out, index_out, semantic_reps, B, kind, _wrong_kind)     # (_keep: converted semantic reps)
    if B:
        ws = M.empty(lg, B * T * 16, "uint8") if kind == _lib.MEM_DEVICE else None
        _lib.check(lib.dhr_lexical_head(M.device(lg), kind, mode, M.data_ptr(lg), _lib._val_code(lg, bf16=True), B, T, V, ldb, ldt, M.data_ptr(w), T,
                                        M.data_ptr(m), T, dims, remove_dims, p_v, _lib._val_code(value_out), ld_v, *record, M.data_ptr(ws), M.stream(lg)),
                   "dhr_lexical_head")
    return B, V


def lexical_reps(logits, term_weights, attention_mask):
    """-> [B, V] fp32 lexical reps, torch.max((softmax(logits) * term_weights) * attention_mask, dim=-2).values.
    numpy in -> numpy out; torch in -> torch out (same device)."""
    B, V = int(logits.shape[0]), int(logits.shape[-1])
    out = M.empty(logits, (B, V), "float32")
    _run(_lib.LEX_RAW, logits, term_weights, attention_mask, out, None, 0, 0, None)
    return out


def _check_out(value_out, B, cols):
    if int(value_out.shape[0]) != B or int(value_out.shape[1]) < cols:
        raise ValueError("output arrays do not match the batch / dims")


def densify_lexical_into(logits, term_weights, attention_mask, value_out, index_out, dims: int = 768, remove_dims: int = 570, semantic_reps=None):
    """The DHR / DLR branch of encode.py:155-170,179-194 in one op: densify(lexical reps, dims, remove_dims) written into the first `dims`
    columns of the record's value array (fp16 or fp32, rows of width dims + cls_dim) and its index array (uint8, or int16 beyond 256
    groups); semantic_reps [B, cls_dim], if given, into the value columns [dims, dims + cls_dim).  -> (value_out, index_out)."""
    B, V = int(logits.shape[0]), int(logits.shape[-1])
    _densify_check(V, dims, remove_dims)
    cls = 0 if semantic_reps is None else int(semantic_reps.shape[1])
    _check_out(value_out, B, dims + cls)
    _check_out(index_out, B, dims)
    _run(_lib.LEX_DENSIFY, logits, term_weights, attention_mask, value_out, index_out, dims, remove_dims, semantic_reps)
    return value_out, index_out


def aggregate_lexical_into(logits, term_weights, attention_mask, value_out, agg_dim: int = 640, full: bool = True, semantic_reps=None):
    """The `agg` branch of encode.py:149-153,174-178 in one op: aggregate(lexical reps, agg_dim, full) (+ merge_reps with semantic_reps)
    written into the record's value array [B, >= agg_dim + cls_dim] (fp16 or fp32).  -> value_out."""
    B, V = int(logits.shape[0]), int(logits.shape[-1])
    remove, _ = _agg_geometry(B, V, agg_dim, full)
    cls = 0 if semantic_reps is None else int(semantic_reps.shape[1])
    _check_out(value_out, B, agg_dim + cls)
    _run(_lib.LEX_AGG_FULL if full else _lib.LEX_AGG_SEMI, logits, term_weights, attention_mask, value_out, None, agg_dim, remove, semantic_reps)
    return value_out


def aggregate(lexical_reps, dims: int = 640, remove_dims: int = -198, full: bool = True):
    """tevatron/Aggretriever/utils.py:16-44 on the HIP kernel: [B, V] reps -> [B, dims] in the input dtype.  As in the reference,
    full=True takes remove = cal_remove_dim(2 * dims) and ignores `remove_dims`; full=False removes cal_remove_dim(dims) columns.
    numpy in -> numpy out; torch in -> torch out (same device, torch's current stream, complete on return)."""
    del remove_dims                                     # (the reference overwrites it in both branches)
    if len(lexical_reps.shape) != 2:
        raise ValueError('Input lexical representation shape should be 2 (batch, vocab), but the input shape is {}'.format(len(lexical_reps.shape)))
    B, V = int(lexical_reps.shape[0]), int(lexical_reps.shape[1])
    remove, _ = _agg_geometry(B, V, dims, full)
    lib = _lib.load()
    src = M.values(lexical_reps if M.is_np(lexical_reps) else lexical_reps.detach())
    src = np.ascontiguousarray(src) if M.is_np(src) else src.contiguous()
    out = M.empty(src, (B, dims), src.dtype)
    _lib.check(lib.dhr_aggregate(M.device(src), M.mem_kind(src), M.data_ptr(src), _lib._val_code(src), V, B, V, dims, remove, 1 if full else 0,
                                 M.data_ptr(out), _lib._val_code(out), dims, M.stream(src)), "dhr_aggregate")
    return M.cast(out, lexical_reps.dtype)
