#!/usr/bin/env python
"""What the lexical heads (lexical.hip, lexical_train.hip, lexical_proj.hip, lexical_proj_train.hip and the four Python modules on them) COMPUTE
and how they ANSWER bad arguments, pinned to the commit before their host code was rewritten around one argument check, one workspace layout
and one error style.  Two recordings:

  tests/golden/lexical_entry_points.json       collect_checks(): every validation exit of the seven C entry points that is reached before the
                                               first HIP call -- (status, exact dhr_last_error text) --, the three workspace functions over a
                                               grid, and the exceptions (type, exact text) of bad calls to the public Python functions.  No GPU.
  tests/golden/lexical_entry_points_gpu.json   collect_gpu(): SHA-256 digests of every output of the four modules on shapes that cross every
                                               tile, chunk and slab boundary.  The ops document bit-identical repeats, so the recording is
                                               made twice and both must agree (--verify); there is no list of dropped fields.

Run at the commit whose behaviour is to be pinned:
  python tests/golden/make_golden_lexical_entry_points.py --checks          writes the first file
  python tests/golden/make_golden_lexical_entry_points.py --gpu [--out F]   writes the second (to F)
  python tests/golden/make_golden_lexical_entry_points.py --gpu --verify [--out F]   recomputes it and lists every field that differs from F"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATH_CHECKS = os.path.join(HERE, "lexical_entry_points.json")
PATH_GPU = os.path.join(HERE, "lexical_entry_points_gpu.json")

HOST, DEVICE = 0, 1
F16, F32, BF16 = 0, 1, 2
U8, I16 = 1, 3
RAW, DENSIFY, AGG_FULL, AGG_SEMI = 0, 1, 2, 3
GRID_B, GRID_T, GRID_V, GRID_H = (0, 1, 3, 700, 70000), (1, 6, 512, 32767, 32768), (1, 256, 257, 300, 30522), (8, 72, 768, 776, 1024, 1032)
SEED = 4711
# shape A: two vocabulary tiles (the second partial), two 64-column chunks of H (the second partial)
B, L, SKIP, V, H = 3, 7, 1, 300, 72
T = L - SKIP
MASK = np.array([[1, 1, 1, 1, 1, 1], [1, 1, 0, 1, 0, 0], [1, 0, 0, 0, 0, 0]], np.int64)
DIMS, REMOVE, AGG_DIM, CLS = 96, 12, 23, 5                                  # densify: (300 - 12) / 96 = 3 groups; aggregate: 6 (full, 24 removed) and 13 (semi, 1 removed) groups


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------ validation exits of the C entry points (CPU)
def _caller(fn, names, defaults):
    """-> make(**changes): a thunk that calls fn with the defaults and the changes, by argument name"""
    names = names.split()
    assert set(names) == set(defaults), set(names) ^ set(defaults)

    def make(**kw):
        assert not set(kw) - set(names), set(kw) - set(names)
        args = dict(defaults, **kw)
        return lambda: fn(*[args[n] for n in names])
    return make


def _check_cases(lib):
    """-> ({name: thunk}, keepalive); a thunk makes one call that must return before the library touches the device"""
    buf = np.zeros(1 << 16, np.uint8)                                       # every pointer below: never dereferenced (256-byte aligned, + 8 is not)
    p = (buf.ctypes.data + 255) & ~255
    head = _caller(lib.dhr_lexical_head,
                   "device mem_kind mode logits logits_dtype batch n_tokens vocab ld_batch ld_token term_weights ld_weights mask ld_mask dims remove_dims "
                   "out_value out_value_dtype ld_value out_index index_dtype ld_index cls cls_dtype ld_cls cls_dim workspace stream",
                   dict(device=0, mem_kind=HOST, mode=RAW, logits=p, logits_dtype=F32, batch=2, n_tokens=3, vocab=64, ld_batch=192, ld_token=64, term_weights=p,
                        ld_weights=3, mask=p, ld_mask=3, dims=0, remove_dims=0, out_value=p, out_value_dtype=F32, ld_value=64, out_index=None, index_dtype=0,
                        ld_index=0, cls=None, cls_dtype=F16, ld_cls=0, cls_dim=0, workspace=None, stream=None))
    dens = dict(mode=DENSIFY, dims=8, ld_value=8, out_index=p, index_dtype=U8, ld_index=8)               # 64 / 8 = 8 groups
    agg = _caller(lib.dhr_aggregate, "device mem_kind lexical value_dtype ld batch vocab dims remove_dims full out out_dtype ld_out stream",
                  dict(device=0, mem_kind=HOST, lexical=p, value_dtype=F32, ld=64, batch=2, vocab=64, dims=8, remove_dims=0, full=1, out=p, out_dtype=F32,
                       ld_out=8, stream=None))
    train = _caller(lib.dhr_lexical_head_train,
                    "device mem_kind logits value_dtype batch n_tokens skip_tokens vocab ld_batch ld_token term_weights ld_weights mask ld_mask out_reps ld_reps "
                    "out_tokens ld_tokens workspace stream",
                    dict(device=0, mem_kind=DEVICE, logits=p, value_dtype=F16, batch=2, n_tokens=3, skip_tokens=1, vocab=64, ld_batch=256, ld_token=64,
                         term_weights=p, ld_weights=3, mask=p, ld_mask=3, out_reps=p, ld_reps=64, out_tokens=p, ld_tokens=64, workspace=p, stream=None))
    back = _caller(lib.dhr_lexical_head_backward,
                   "device mem_kind logits value_dtype batch n_tokens skip_tokens vocab ld_batch ld_token grad_reps ld_grad_reps tokens ld_tokens workspace "
                   "grad_logits ld_grad_batch ld_grad_token grad_weights ld_grad_weights stream",
                   dict(device=0, mem_kind=DEVICE, logits=p, value_dtype=F16, batch=2, n_tokens=3, skip_tokens=1, vocab=64, ld_batch=256, ld_token=64, grad_reps=p,
                        ld_grad_reps=64, tokens=p, ld_tokens=64, workspace=p, grad_logits=p, ld_grad_batch=256, ld_grad_token=64, grad_weights=p,
                        ld_grad_weights=3, stream=None))
    n_ws = int(lib.dhr_lexical_proj_workspace(2, 3, 64, RAW))
    proj = _caller(lib.dhr_lexical_proj_head,
                   "device mem_kind mode hidden value_dtype batch n_tokens hidden_dim ld_batch ld_token weight vocab ld_weight bias bias_dtype term_weights "
                   "ld_weights mask ld_mask dims remove_dims out_value out_value_dtype ld_value out_index index_dtype ld_index cls cls_dtype ld_cls cls_dim "
                   "workspace workspace_bytes stream",
                   dict(device=0, mem_kind=DEVICE, mode=RAW, hidden=p, value_dtype=F16, batch=2, n_tokens=3, hidden_dim=16, ld_batch=48, ld_token=16, weight=p,
                        vocab=64, ld_weight=16, bias=p, bias_dtype=F32, term_weights=p, ld_weights=3, mask=p, ld_mask=3, dims=0, remove_dims=0, out_value=p,
                        out_value_dtype=F32, ld_value=64, out_index=None, index_dtype=0, ld_index=0, cls=None, cls_dtype=F16, ld_cls=0, cls_dim=0, workspace=p,
                        workspace_bytes=n_ws, stream=None))
    n_tws = int(lib.dhr_lexical_proj_train_workspace(2, 3, 64, 16))
    common = ("device mem_kind hidden value_dtype batch n_tokens skip_tokens hidden_dim ld_batch ld_token weight vocab ld_weight bias bias_dtype term_weights "
              "ld_weights mask ld_mask ")
    common_defaults = dict(device=0, mem_kind=DEVICE, hidden=p, value_dtype=F16, batch=2, n_tokens=3, skip_tokens=1, hidden_dim=16, ld_batch=64, ld_token=16,
                           weight=p, vocab=64, ld_weight=16, bias=p, bias_dtype=F32, term_weights=p, ld_weights=3, mask=p, ld_mask=3)
    ptrain = _caller(lib.dhr_lexical_proj_train, common + "out_reps ld_reps out_tokens ld_tokens out_pwin ld_pwin workspace workspace_bytes stream",
                     dict(common_defaults, out_reps=p, ld_reps=64, out_tokens=p, ld_tokens=64, out_pwin=p, ld_pwin=64, workspace=p, workspace_bytes=n_tws,
                          stream=None))
    pback = _caller(lib.dhr_lexical_proj_backward,
                    common + "grad_reps ld_grad_reps tokens ld_tokens pwin ld_pwin workspace workspace_bytes grad_hidden grad_hidden_dtype ld_grad_batch "
                    "ld_grad_token grad_weight grad_weight_dtype ld_grad_weight grad_bias grad_bias_dtype grad_term_weights ld_grad_term_weights stream",
                    dict(common_defaults, grad_reps=p, ld_grad_reps=64, tokens=p, ld_tokens=64, pwin=p, ld_pwin=64, workspace=p, workspace_bytes=n_tws,
                         grad_hidden=p, grad_hidden_dtype=F16, ld_grad_batch=64, ld_grad_token=16, grad_weight=p, grad_weight_dtype=F16, ld_grad_weight=16,
                         grad_bias=p, grad_bias_dtype=F32, grad_term_weights=p, ld_grad_term_weights=3, stream=None))
    big = 1 << 30
    cases = {}

    def record_rules(prefix, fn, value_dt):
        """the record rules dhr_lexical_head and dhr_lexical_proj_head share, in the order of the checks (geometry() first)"""
        d = dict(dens, out_value_dtype=value_dt)
        cases.update({
            prefix + "mode_bad": fn(mode=4, dims=8),
            prefix + "mode_negative": fn(mode=-1, dims=8),
            prefix + "dims_zero": fn(**dict(d, dims=0)),
            prefix + "agg_full_dims_too_large": fn(mode=AGG_FULL, dims=(1 << 29) + 1, ld_value=big),
            prefix + "remove_negative_densify": fn(**dict(d, remove_dims=-8)),
            prefix + "remove_negative_agg_semi": fn(mode=AGG_SEMI, dims=8, remove_dims=-8, ld_value=8),
            prefix + "densify_not_divisible": fn(**dict(d, dims=7, ld_value=7, ld_index=7)),
            prefix + "densify_remove_all": fn(**dict(d, remove_dims=64)),
            prefix + "agg_full_not_divisible": fn(mode=AGG_FULL, dims=5, ld_value=5),
            prefix + "agg_semi_not_divisible": fn(mode=AGG_SEMI, dims=7, ld_value=7),
            prefix + "over_32767_groups": fn(**dict(d, vocab=40000, ld_token=40000, ld_batch=120000, dims=1, ld_value=1, ld_index=1, index_dtype=I16)),
            prefix + "ld_value_short_raw": fn(ld_value=63),
            prefix + "ld_value_short_densify": fn(**dict(d, ld_value=7)),
            prefix + "ld_value_short_of_cls": fn(**dict(d, ld_value=10, cls=p, ld_cls=3, cls_dim=3)),
            prefix + "cls_null": fn(**dict(d, ld_value=11, cls=None, ld_cls=3, cls_dim=3)),
            prefix + "cls_dtype_bf16": fn(**dict(d, ld_value=11, cls=p, cls_dtype=BF16, ld_cls=3, cls_dim=3)),
            prefix + "cls_ld_short": fn(**dict(d, ld_value=11, cls=p, ld_cls=2, cls_dim=3)),
            prefix + "index_null": fn(**dict(d, out_index=None)),
            prefix + "index_dtype_none": fn(**dict(d, index_dtype=0)),
            prefix + "index_dtype_i8": fn(**dict(d, index_dtype=2)),
            prefix + "u8_over_256_groups": fn(**dict(d, vocab=600, ld_token=600, ld_batch=1800, dims=2, ld_value=2, ld_index=2)),
            prefix + "ld_index_short": fn(**dict(d, ld_index=7)),
            prefix + "agg_full_negative_remove_is_ok_with_empty_batch": fn(mode=AGG_FULL, dims=5, remove_dims=-6, ld_value=5, batch=0),
            prefix + "empty_batch_is_ok": fn(batch=0),
            prefix + "empty_batch_densify_is_ok": fn(**dict(d, batch=0)),
            # two rules at once
            prefix + "geometry_beats_ld_value": fn(**dict(d, dims=7, ld_value=3)),
            prefix + "ld_value_beats_null_index": fn(**dict(d, out_index=None, ld_value=7)),
            prefix + "ld_value_beats_cls": fn(**dict(d, ld_value=7, cls=None, cls_dim=3)),
            prefix + "cls_beats_null_index": fn(**dict(d, ld_value=11, cls=None, cls_dim=3, ld_cls=3, out_index=None)),
            prefix + "null_index_beats_index_dtype": fn(**dict(d, out_index=None, index_dtype=2)),
            prefix + "index_dtype_beats_ld_index": fn(**dict(d, index_dtype=2, ld_index=7)),
            prefix + "group_count_beats_ld_index": fn(**dict(d, vocab=600, ld_token=600, ld_batch=1800, dims=2, ld_value=2, ld_index=1)),
            prefix + "ld_index_beats_empty_batch": fn(**dict(d, ld_index=7, batch=0)),
            prefix + "sizes_beat_geometry": fn(**dict(d, dims=7, ld_mask=2)),
        })

    def proj_record(**kw):                                                  # the projection's rows are hidden_dim wide, whatever the vocabulary
        kw.pop("ld_token", None)
        kw.pop("ld_batch", None)
        return proj(**kw)

    record_rules("head_", head, F16)
    record_rules("proj_", proj_record, F16)
    cases.update({
        # ---- dhr_lexical_head, what stands in front of the record rules
        "head_null_logits": head(logits=None),
        "head_null_term_weights": head(term_weights=None),
        "head_null_mask": head(mask=None),
        "head_null_out_value": head(out_value=None),
        "head_mem_kind": head(mem_kind=7),
        "head_logits_dtype": head(logits_dtype=3),
        "head_out_value_dtype_bf16": head(out_value_dtype=BF16),
        "head_batch_negative": head(batch=-1),
        "head_no_tokens": head(n_tokens=0),
        "head_vocab_zero": head(vocab=0),
        "head_ld_token_short": head(ld_token=63),
        "head_ld_batch_short": head(ld_batch=191),
        "head_ld_weights_short": head(ld_weights=2),
        "head_ld_mask_short": head(ld_mask=2),
        "head_cls_dim_negative": head(cls_dim=-1),
        "head_too_many_rows": head(batch=1 << 30, n_tokens=2, ld_batch=128, ld_weights=2, ld_mask=2),
        "head_bf16_logits_from_host_is_checked_later": head(logits_dtype=BF16, batch=0),
        "head_null_beats_mem_kind": head(logits=None, mem_kind=7),
        "head_null_beats_dtype": head(mask=None, logits_dtype=3),
        "head_mem_kind_beats_dtype": head(mem_kind=7, logits_dtype=3),
        "head_dtype_beats_sizes": head(out_value_dtype=BF16, ld_token=63),
        "head_densify_null_index_and_ld_value_short": head(**dict(dens, out_index=None, ld_value=7)),
        # ---- dhr_aggregate
        "agg_null_lexical": agg(lexical=None),
        "agg_null_out": agg(out=None),
        "agg_mem_kind": agg(mem_kind=7),
        "agg_value_dtype_bf16": agg(value_dtype=BF16),
        "agg_out_dtype": agg(out_dtype=3),
        "agg_batch_negative": agg(batch=-1),
        "agg_vocab_zero": agg(vocab=0),
        "agg_ld_short": agg(ld=63),
        "agg_ld_out_short": agg(ld_out=7),
        "agg_dims_zero": agg(dims=0, ld_out=0),
        "agg_full_dims_too_large": agg(dims=(1 << 29) + 1, ld_out=big),
        "agg_semi_remove_negative": agg(full=0, remove_dims=-8),
        "agg_full_not_divisible": agg(dims=5, ld_out=5),
        "agg_semi_not_divisible": agg(full=0, dims=7, ld_out=7),
        "agg_full_pads_with_negative_remove": agg(dims=5, remove_dims=-6, ld_out=5, batch=0),
        "agg_over_32767_groups": agg(full=0, vocab=40000, ld=40000, dims=1, ld_out=1),
        "agg_empty_batch_is_ok": agg(batch=0),
        "agg_null_beats_mem_kind": agg(out=None, mem_kind=7),
        "agg_mem_kind_beats_dtype": agg(mem_kind=7, out_dtype=3),
        "agg_dtype_beats_sizes": agg(value_dtype=BF16, ld=63),
        "agg_sizes_beat_geometry": agg(ld_out=4, dims=5),
        "agg_geometry_beats_empty_batch": agg(dims=5, ld_out=5, batch=0),
        # ---- dhr_lexical_head_train: its own pointers, check_head, its own strides
        "train_null_term_weights": train(term_weights=None),
        "train_null_mask": train(mask=None),
        "train_null_out_reps": train(out_reps=None),
        "train_null_out_tokens": train(out_tokens=None),
        "train_null_logits": train(logits=None),
        "train_null_workspace": train(workspace=None),
        "train_mem_kind": train(mem_kind=7),
        "train_value_dtype": train(value_dtype=3),
        "train_batch_negative": train(batch=-1),
        "train_no_tokens": train(n_tokens=0),
        "train_vocab_zero": train(vocab=0),
        "train_skip_negative": train(skip_tokens=-1),
        "train_skip_too_large": train(skip_tokens=32768, ld_batch=big),
        "train_ld_token_short": train(ld_token=63),
        "train_ld_batch_short_of_the_skipped_token": train(ld_batch=255),
        "train_too_many_rows": train(batch=1 << 30, n_tokens=2, ld_batch=192),
        "train_over_32767_tokens": train(n_tokens=32768, ld_batch=big, ld_weights=32768, ld_mask=32768),
        "train_host_memory": train(mem_kind=HOST),
        "train_ld_weights_short": train(ld_weights=2),
        "train_ld_mask_short": train(ld_mask=2),
        "train_ld_reps_short": train(ld_reps=63),
        "train_ld_tokens_short": train(ld_tokens=63),
        "train_empty_batch_is_ok": train(batch=0),
        "train_own_null_beats_null_logits": train(mask=None, logits=None),
        "train_null_beats_mem_kind": train(workspace=None, mem_kind=7),
        "train_dtype_beats_sizes": train(value_dtype=3, ld_token=63),
        "train_sizes_beat_token_limit": train(n_tokens=32768, ld_batch=255),
        "train_token_limit_beats_host_memory": train(n_tokens=32768, ld_batch=big, mem_kind=HOST),
        "train_host_memory_beats_own_strides": train(mem_kind=HOST, ld_reps=63),
        "train_fp32_from_host_memory": train(value_dtype=F32, mem_kind=HOST),
        "train_strides_beat_empty_batch": train(ld_weights=2, batch=0),
        # ---- dhr_lexical_head_backward
        "back_null_grad_reps": back(grad_reps=None),
        "back_null_tokens": back(tokens=None),
        "back_null_logits": back(logits=None),
        "back_null_workspace": back(workspace=None),
        "back_mem_kind": back(mem_kind=7),
        "back_value_dtype": back(value_dtype=3),
        "back_skip_negative": back(skip_tokens=-1),
        "back_ld_batch_short": back(ld_batch=255),
        "back_over_32767_tokens": back(n_tokens=32768, ld_batch=big, ld_grad_batch=big, ld_grad_weights=32768),
        "back_host_memory": back(mem_kind=HOST),
        "back_ld_grad_reps_short": back(ld_grad_reps=63),
        "back_ld_tokens_short": back(ld_tokens=63),
        "back_ld_grad_weights_short": back(ld_grad_weights=2),
        "back_ld_grad_weights_short_without_the_gradient_is_ok": back(grad_weights=None, ld_grad_weights=0, batch=0),
        "back_ld_grad_token_short": back(ld_grad_token=63),
        "back_ld_grad_batch_short": back(ld_grad_batch=255),
        "back_empty_batch_is_ok": back(batch=0),
        "back_no_gradient_wanted_is_ok": back(grad_logits=None, grad_weights=None),
        "back_own_null_beats_null_workspace": back(tokens=None, workspace=None),
        "back_host_memory_beats_own_strides": back(mem_kind=HOST, ld_grad_reps=63),
        "back_strides_beat_no_gradient_wanted": back(grad_logits=None, grad_weights=None, ld_tokens=63),
        # ---- dhr_lexical_proj_head, what stands in front of the record rules, and behind them
        "proj_null_hidden": proj(hidden=None),
        "proj_null_weight": proj(weight=None),
        "proj_null_term_weights": proj(term_weights=None),
        "proj_null_mask": proj(mask=None),
        "proj_null_out_value": proj(out_value=None),
        "proj_null_bias_is_allowed": proj(bias=None, batch=0),
        "proj_host_memory": proj(mem_kind=HOST),
        "proj_mem_kind": proj(mem_kind=7),
        "proj_value_dtype": proj(value_dtype=3),
        "proj_out_value_dtype_bf16": proj(out_value_dtype=BF16),
        "proj_bias_dtype": proj(bias_dtype=3),
        "proj_bias_dtype_without_a_bias": proj(bias=None, bias_dtype=3, batch=0),
        "proj_fp32_operands": proj(value_dtype=F32),
        "proj_bf16_bias_fp16_operands": proj(bias_dtype=BF16),
        "proj_bf16_bias_bf16_operands": proj(bias_dtype=BF16, value_dtype=BF16, batch=0),
        "proj_batch_negative": proj(batch=-1),
        "proj_no_tokens": proj(n_tokens=0),
        "proj_vocab_zero": proj(vocab=0),
        "proj_hidden_dim_zero": proj(hidden_dim=0),
        "proj_ld_token_short": proj(ld_token=15),
        "proj_ld_batch_short": proj(ld_batch=47),
        "proj_ld_weight_short": proj(ld_weight=15),
        "proj_ld_weights_short": proj(ld_weights=2),
        "proj_ld_mask_short": proj(ld_mask=2),
        "proj_cls_dim_negative": proj(cls_dim=-1),
        "proj_workspace_bytes_negative": proj(workspace_bytes=-1),
        "proj_too_many_rows": proj(batch=1 << 30, n_tokens=2, ld_batch=32, ld_weights=2, ld_mask=2),
        "proj_hidden_dim_not_multiple_of_8": proj(hidden_dim=12),
        "proj_hidden_dim_1032_is_not_refused_here": proj(hidden_dim=1032, ld_token=1032, ld_batch=3096, ld_weight=1032, batch=0),
        "proj_32768_tokens_are_not_refused_here": proj(n_tokens=32768, ld_batch=big, ld_weights=32768, ld_mask=32768, batch=0),
        "proj_raw_fp16": proj(out_value_dtype=F16),
        "proj_workspace_null": proj(workspace=None),
        "proj_workspace_short": proj(workspace_bytes=n_ws - 1),
        "proj_workspace_short_for_densify": proj(**dict(dens, out_value_dtype=F16)),
        "proj_workspace_misaligned": proj(workspace=p + 8, workspace_bytes=n_ws + 8),
        "proj_null_beats_host_memory": proj(hidden=None, mem_kind=HOST),
        "proj_null_pointer_and_bad_dtype": proj(weight=None, value_dtype=3),
        "proj_host_memory_beats_fp32_operands": proj(mem_kind=HOST, value_dtype=F32),
        "proj_dtype_beats_fp32_operands": proj(value_dtype=F32, out_value_dtype=BF16),
        "proj_fp32_operands_beat_sizes": proj(value_dtype=F32, ld_token=15),
        "proj_bf16_bias_beats_sizes": proj(bias_dtype=BF16, ld_weight=15),
        "proj_bad_stride_and_hidden_dim_not_multiple_of_8": proj(hidden_dim=12, ld_mask=2),
        "proj_multiple_of_8_beats_geometry": proj(**dict(dens, hidden_dim=12, dims=7)),
        "proj_record_rules_beat_raw_fp16": proj(out_value_dtype=F16, ld_value=63),
        "proj_raw_fp16_beats_empty_batch": proj(out_value_dtype=F16, batch=0),
        "proj_empty_batch_beats_workspace": proj(batch=0, workspace=None, workspace_bytes=0),
        "proj_workspace_short_and_misaligned": proj(workspace=p + 8, workspace_bytes=n_ws - 1),
        # ---- dhr_lexical_proj_train: its own pointers, the operand rules, its own strides, the workspace
        "ptrain_null_out_reps": ptrain(out_reps=None),
        "ptrain_null_out_tokens": ptrain(out_tokens=None),
        "ptrain_null_out_pwin": ptrain(out_pwin=None),
        "ptrain_null_hidden": ptrain(hidden=None),
        "ptrain_null_weight": ptrain(weight=None),
        "ptrain_null_term_weights": ptrain(term_weights=None),
        "ptrain_null_mask": ptrain(mask=None),
        "ptrain_null_bias_is_allowed": ptrain(bias=None, batch=0),
        "ptrain_mem_kind": ptrain(mem_kind=7),
        "ptrain_value_dtype": ptrain(value_dtype=3),
        "ptrain_bias_dtype": ptrain(bias_dtype=3),
        "ptrain_batch_negative": ptrain(batch=-1),
        "ptrain_no_tokens": ptrain(n_tokens=0),
        "ptrain_vocab_zero": ptrain(vocab=0),
        "ptrain_hidden_dim_zero": ptrain(hidden_dim=0),
        "ptrain_skip_negative": ptrain(skip_tokens=-1),
        "ptrain_skip_too_large": ptrain(skip_tokens=32768, ld_batch=big),
        "ptrain_ld_token_short": ptrain(ld_token=15),
        "ptrain_ld_batch_short_of_the_skipped_token": ptrain(ld_batch=63),
        "ptrain_ld_weight_short": ptrain(ld_weight=15),
        "ptrain_ld_weights_short": ptrain(ld_weights=2),
        "ptrain_ld_mask_short": ptrain(ld_mask=2),
        "ptrain_workspace_bytes_negative": ptrain(workspace_bytes=-1),
        "ptrain_too_many_rows_with_the_skipped_ones": ptrain(batch=(1 << 31) // 3 + 1, n_tokens=2, ld_batch=48, ld_weights=2, ld_mask=2),
        "ptrain_hidden_dim_not_multiple_of_8": ptrain(hidden_dim=12),
        "ptrain_over_32767_tokens": ptrain(n_tokens=32768, ld_batch=big, ld_weights=32768, ld_mask=32768),
        "ptrain_hidden_dim_1032": ptrain(hidden_dim=1032, ld_token=1032, ld_batch=4128, ld_weight=1032),
        "ptrain_fp32_operands": ptrain(value_dtype=F32),
        "ptrain_bf16_bias_fp16_operands": ptrain(bias_dtype=BF16),
        "ptrain_host_memory": ptrain(mem_kind=HOST),
        "ptrain_ld_reps_short": ptrain(ld_reps=63),
        "ptrain_ld_tokens_short": ptrain(ld_tokens=63),
        "ptrain_ld_pwin_short": ptrain(ld_pwin=63),
        "ptrain_empty_batch_is_ok": ptrain(batch=0),
        "ptrain_workspace_null": ptrain(workspace=None),
        "ptrain_workspace_short": ptrain(workspace_bytes=n_tws - 1),
        "ptrain_workspace_misaligned": ptrain(workspace=p + 8),
        "ptrain_own_null_beats_null_hidden": ptrain(out_pwin=None, hidden=None),
        "ptrain_null_beats_mem_kind": ptrain(mask=None, mem_kind=7),
        "ptrain_mem_kind_beats_dtype": ptrain(mem_kind=7, value_dtype=3),
        "ptrain_dtype_beats_sizes": ptrain(bias_dtype=3, hidden_dim=0),
        "ptrain_sizes_beat_multiple_of_8": ptrain(hidden_dim=12, ld_weights=2),
        "ptrain_multiple_of_8_beats_token_limit": ptrain(hidden_dim=12, n_tokens=32768, ld_batch=big, ld_weights=32768, ld_mask=32768),
        "ptrain_token_limit_beats_hidden_limit": ptrain(n_tokens=32768, hidden_dim=1032, ld_token=1032, ld_batch=big, ld_weight=1032, ld_weights=32768, ld_mask=32768),
        "ptrain_hidden_limit_beats_fp32_operands": ptrain(hidden_dim=1032, ld_token=1032, ld_batch=4128, ld_weight=1032, value_dtype=F32),
        "ptrain_fp32_operands_beat_bf16_bias": ptrain(value_dtype=F32, bias_dtype=BF16),
        "ptrain_sizes_beat_fp32_operands": ptrain(value_dtype=F32, ld_token=15),
        "ptrain_multiple_of_8_beats_bf16_bias": ptrain(hidden_dim=12, bias_dtype=BF16),
        "ptrain_fp32_operands_and_host_memory": ptrain(value_dtype=F32, mem_kind=HOST),
        "ptrain_bf16_bias_beats_host_memory": ptrain(bias_dtype=BF16, mem_kind=HOST),
        "ptrain_host_memory_beats_own_strides": ptrain(mem_kind=HOST, ld_pwin=63),
        "ptrain_strides_beat_empty_batch": ptrain(ld_reps=63, batch=0),
        "ptrain_empty_batch_beats_workspace": ptrain(batch=0, workspace=None, workspace_bytes=0),
        "ptrain_workspace_short_and_misaligned": ptrain(workspace=p + 8, workspace_bytes=n_tws - 1),
        # ---- dhr_lexical_proj_backward
        "pback_null_grad_reps": pback(grad_reps=None),
        "pback_null_tokens": pback(tokens=None),
        "pback_null_pwin": pback(pwin=None),
        "pback_null_hidden": pback(hidden=None),
        "pback_mem_kind": pback(mem_kind=7),
        "pback_value_dtype": pback(value_dtype=3),
        "pback_hidden_dim_not_multiple_of_8": pback(hidden_dim=12),
        "pback_over_32767_tokens": pback(n_tokens=32768, ld_batch=big, ld_weights=32768, ld_mask=32768),
        "pback_hidden_dim_1032": pback(hidden_dim=1032, ld_token=1032, ld_batch=4128, ld_weight=1032),
        "pback_fp32_operands": pback(value_dtype=F32),
        "pback_bf16_bias_fp16_operands": pback(bias_dtype=BF16),
        "pback_host_memory": pback(mem_kind=HOST),
        "pback_grad_hidden_dtype": pback(grad_hidden_dtype=3),
        "pback_grad_weight_dtype": pback(grad_weight_dtype=3),
        "pback_grad_bias_dtype": pback(grad_bias_dtype=3),
        "pback_grad_dtype_of_an_unwanted_gradient_is_ok": pback(grad_weight=None, grad_weight_dtype=3, batch=0),
        "pback_bf16_grad_hidden_fp16_operands": pback(grad_hidden_dtype=BF16),
        "pback_bf16_grad_weight_fp16_operands": pback(grad_weight_dtype=BF16),
        "pback_bf16_grad_bias_fp16_operands": pback(grad_bias_dtype=BF16),
        "pback_bf16_gradients_bf16_operands": pback(value_dtype=BF16, grad_hidden_dtype=BF16, grad_weight_dtype=BF16, grad_bias_dtype=BF16, batch=0),
        "pback_ld_grad_reps_short": pback(ld_grad_reps=63),
        "pback_ld_tokens_short": pback(ld_tokens=63),
        "pback_ld_pwin_short": pback(ld_pwin=63),
        "pback_ld_grad_term_weights_short": pback(ld_grad_term_weights=2),
        "pback_ld_grad_weight_short": pback(ld_grad_weight=15),
        "pback_ld_grad_token_short": pback(ld_grad_token=15),
        "pback_ld_grad_batch_short": pback(ld_grad_batch=63),
        "pback_empty_batch_is_ok": pback(batch=0),
        "pback_no_gradient_wanted_is_ok": pback(grad_hidden=None, grad_weight=None, grad_bias=None, grad_term_weights=None, workspace=None),
        "pback_workspace_null": pback(workspace=None),
        "pback_workspace_short": pback(workspace_bytes=n_tws - 1),
        "pback_workspace_misaligned": pback(workspace=p + 8),
        "pback_own_null_beats_null_weight": pback(pwin=None, weight=None),
        "pback_sizes_beat_fp32_operands": pback(value_dtype=F32, ld_weight=15),
        "pback_operand_rules_beat_grad_dtype": pback(mem_kind=HOST, grad_hidden_dtype=3),
        "pback_grad_dtype_beats_bf16_gradient": pback(grad_hidden_dtype=BF16, grad_bias_dtype=3),
        "pback_bf16_gradient_beats_strides": pback(grad_weight_dtype=BF16, ld_pwin=63),
        "pback_strides_beat_no_gradient_wanted": pback(grad_hidden=None, grad_weight=None, grad_bias=None, grad_term_weights=None, ld_grad_reps=63),
        "pback_workspace_short_and_misaligned": pback(workspace=p + 8, workspace_bytes=n_tws - 1),
    })
    return cases, buf


def _workspace_grid(lib):
    """the three workspace functions (pure host code: the layout totals) over the grid, in the order of the nested loops"""
    out = {"proj": [], "proj_train": [], "head_train": []}
    for b in GRID_B:
        for t in GRID_T:
            out["head_train"].append(int(lib.dhr_lexical_head_train_workspace(b, t)))
            for v in GRID_V:
                for mode in (RAW, DENSIFY, AGG_FULL, AGG_SEMI):
                    out["proj"].append(int(lib.dhr_lexical_proj_workspace(b, t, v, mode)))
                for h in GRID_H:
                    out["proj_train"].append(int(lib.dhr_lexical_proj_train_workspace(b, t, v, h)))
    out["extra"] = {"proj_negative_batch": int(lib.dhr_lexical_proj_workspace(-1, 6, 300, RAW)), "proj_no_tokens": int(lib.dhr_lexical_proj_workspace(3, 0, 300, RAW)),
                    "proj_no_vocab": int(lib.dhr_lexical_proj_workspace(3, 6, 0, RAW)), "proj_too_many_rows": int(lib.dhr_lexical_proj_workspace(1 << 30, 2, 300, RAW)),
                    "proj_train_h_12": int(lib.dhr_lexical_proj_train_workspace(3, 6, 300, 12)), "proj_train_h_0": int(lib.dhr_lexical_proj_train_workspace(3, 6, 300, 0)),
                    "proj_train_negative_batch": int(lib.dhr_lexical_proj_train_workspace(-1, 6, 300, 72)),
                    "head_train_negative_batch": int(lib.dhr_lexical_head_train_workspace(-1, 6))}
    return out


# ------------------------------------------------------------------------------------------------ bad calls to the Python modules (CPU)
def _python_cases():
    """-> {name: thunk}; every thunk raises before the library touches the device (numpy arrays and torch CPU tensors only)"""
    import torch
    from dhr_amd import lexical as LX, lexical_proj as LP, lexical_proj_train as LPT, lexical_train as LT
    f = np.float32
    lg, w, m = np.zeros((2, 3, 8), f), np.ones((2, 3), f), np.ones((2, 3), np.int64)
    val, idx = np.zeros((2, 4), np.float16), np.zeros((2, 4), np.uint8)
    tlg, tw, tm = torch.zeros((2, 4, 8), dtype=torch.float16), torch.ones((2, 3)), torch.ones((2, 3), dtype=torch.long)
    th, tW, tb = torch.zeros((2, 4, 16), dtype=torch.float16), torch.zeros((8, 16), dtype=torch.float16), torch.zeros(8)
    bf = torch.bfloat16
    cases = {
        # ---- dhr_amd.lexical
        "lexical_logits_rank": lambda: LX.lexical_reps(np.zeros((2, 8), f), w, m),
        "lexical_no_tokens": lambda: LX.lexical_reps(np.zeros((2, 0, 8), f), np.zeros((2, 0), f), np.zeros((2, 0), f)),
        "lexical_logits_dtype_numpy": lambda: LX.lexical_reps(lg.astype(np.int32), w, m),
        "lexical_logits_dtype_torch": lambda: LX.lexical_reps(torch.zeros((2, 3, 8), dtype=torch.int32), tw, tm),
        "lexical_logits_float64": lambda: LX.lexical_reps(lg.astype(np.float64), w, m),
        "lexical_bf16_on_the_cpu": lambda: LX.lexical_reps(torch.zeros((2, 3, 8), dtype=bf), tw, tm),
        "lexical_term_weights_shape_numpy": lambda: LX.lexical_reps(lg, np.ones((2, 4), f), m),
        "lexical_mask_shape_numpy": lambda: LX.lexical_reps(lg, w, np.ones((3, 3), np.int64)),
        "lexical_term_weights_shape_torch": lambda: LX.lexical_reps(torch.zeros((2, 3, 8)), torch.ones((2, 4)), tm),
        "lexical_torch_logits_numpy_weights": lambda: LX.lexical_reps(torch.zeros((2, 3, 8)), w, tm),
        "lexical_densify_not_divisible": lambda: LX.densify_lexical_into(lg, w, m, val, idx, dims=3, remove_dims=0),
        "lexical_densify_value_rows": lambda: LX.densify_lexical_into(lg, w, m, np.zeros((3, 4), np.float16), idx, dims=4, remove_dims=0),
        "lexical_densify_value_cols_short_of_cls": lambda: LX.densify_lexical_into(lg, w, m, val, idx, dims=4, remove_dims=0, semantic_reps=np.zeros((2, 2), f)),
        "lexical_densify_index_cols": lambda: LX.densify_lexical_into(lg, w, m, val, np.zeros((2, 3), np.uint8), dims=4, remove_dims=0),
        "lexical_densify_value_not_2d": lambda: LX.densify_lexical_into(lg, w, m, np.zeros((2, 4, 1), np.float16), idx, dims=4, remove_dims=0),
        "lexical_densify_value_not_contiguous": lambda: LX.densify_lexical_into(lg, w, m, np.zeros((2, 8), np.float16)[:, ::2], idx, dims=4, remove_dims=0),
        "lexical_densify_index_dtype": lambda: LX.densify_lexical_into(lg, w, m, val, np.zeros((2, 4), np.int32), dims=4, remove_dims=0),
        "lexical_densify_index_not_contiguous": lambda: LX.densify_lexical_into(lg, w, m, val, np.zeros((2, 8), np.uint8)[:, ::2], dims=4, remove_dims=0),
        "lexical_densify_semantic_batch": lambda: LX.densify_lexical_into(lg, w, m, np.zeros((2, 6), np.float16), idx, dims=4, remove_dims=0,
                                                                         semantic_reps=np.zeros((3, 2), f)),
        "lexical_densify_semantic_rank": lambda: LX.densify_lexical_into(lg, w, m, np.zeros((2, 6), np.float16), idx, dims=4, remove_dims=0,
                                                                        semantic_reps=np.zeros((2, 2, 1), f)),
        "lexical_densify_rank_beats_output_rules": lambda: LX.densify_lexical_into(np.zeros((2, 8), f), w, m, np.zeros((2, 4, 1), np.float16), idx, dims=4,
                                                                                  remove_dims=0),
        "lexical_aggregate_semi_negative_remove": lambda: LX.aggregate_lexical_into(lg, w, m, np.zeros((2, 1700), f), agg_dim=1700, full=False),
        "lexical_aggregate_into_not_divisible": lambda: LX.aggregate_lexical_into(lg, w, m, np.zeros((2, 2), f), agg_dim=2, full=True),
        "lexical_aggregate_into_value_cols": lambda: LX.aggregate_lexical_into(np.zeros((2, 3, 10), f), w, m, np.zeros((2, 1), f), agg_dim=2, full=True),
        "lexical_aggregate_into_empty_batch": lambda: LX.aggregate_lexical_into(np.zeros((0, 3, 8), f), np.zeros((0, 3), f), np.zeros((0, 3), f), np.zeros((0, 2), f),
                                                                             agg_dim=2),
        "lexical_aggregate_rank": lambda: LX.aggregate(np.zeros((2, 3, 8), f), dims=2),
        "lexical_aggregate_empty": lambda: LX.aggregate(np.zeros((0, 8), f), dims=2),
        "lexical_aggregate_not_divisible": lambda: LX.aggregate(np.zeros((2, 2), f), dims=3, full=False),
        # ---- dhr_amd.lexical_proj: no host path
        "proj_numpy_hidden": lambda: LP.lexical_reps(np.zeros((2, 3, 16), np.float16), tW, tb, tw, tm),
        "proj_cpu_hidden": lambda: LP.lexical_reps(th[:, 1:], tW, tb, tw, tm),
        "proj_list_hidden": lambda: LP.densify_lexical_into([[1.0]], tW, tb, tw, tm, val, idx),
        "proj_densify_not_divisible": lambda: LP.densify_lexical_into(th[:, 1:], tW, tb, tw, tm, val, idx, dims=3, remove_dims=0),
        "proj_densify_value_rows": lambda: LP.densify_lexical_into(th[:, 1:], tW, tb, tw, tm, torch.zeros((3, 4)), idx, dims=4, remove_dims=0),
        "proj_densify_cpu_tensors": lambda: LP.densify_lexical_into(th[:, 1:], tW, tb, tw, tm, torch.zeros((2, 4)), torch.zeros((2, 4), dtype=torch.uint8), dims=4,
                                                                    remove_dims=0),
        "proj_aggregate_not_divisible": lambda: LP.aggregate_lexical_into(th[:, 1:], tW, tb, tw, tm, torch.zeros((2, 2)), agg_dim=2),
        "proj_aggregate_cpu_tensors": lambda: LP.aggregate_lexical_into(th[:, 1:], torch.zeros((10, 16), dtype=torch.float16), None, tw, tm, torch.zeros((2, 2)),
                                                                        agg_dim=2),
        "proj_aggregate_semi_negative_remove": lambda: LP.aggregate_lexical_into(th[:, 1:], tW, None, tw, tm, torch.zeros((2, 1700)), agg_dim=1700, full=False),
        # ---- dhr_amd.lexical_train
        "train_numpy_logits": lambda: LT.lexical_reps(lg, tw, tm),
        "train_numpy_mask": lambda: LT.lexical_reps(tlg, tw, m, skip_tokens=1),
        "train_logits_rank": lambda: LT.lexical_reps(torch.zeros((2, 8)), tw, tm),
        "train_skip_negative": lambda: LT.lexical_reps(tlg, tw, tm, skip_tokens=-1),
        "train_all_skipped": lambda: LT.lexical_reps(tlg, tw, tm, skip_tokens=4),
        "train_no_tokens": lambda: LT.lexical_reps(torch.zeros((2, 0, 8)), torch.zeros((2, 0)), torch.zeros((2, 0))),
        "train_no_vocabulary": lambda: LT.lexical_reps(torch.zeros((2, 4, 0)), tw, tm, skip_tokens=1),
        "train_term_weights_shape": lambda: LT.lexical_reps(tlg, torch.ones((2, 4)), tm, skip_tokens=1),
        "train_term_weights_rank": lambda: LT.lexical_reps(tlg, torch.ones((2, 3, 2)), tm, skip_tokens=1),
        "train_mask_shape": lambda: LT.lexical_reps(tlg, tw, torch.ones((2, 4), dtype=torch.long), skip_tokens=1),
        "train_shape_without_skip": lambda: LT.lexical_reps(tlg, tw, tm),
        "train_over_32767_tokens": lambda: LT.lexical_reps(torch.zeros((1, 32768, 1), dtype=torch.float16), torch.ones((1, 32768)), torch.ones((1, 32768))),
        "train_logits_dtype": lambda: LT.lexical_reps(tlg.double(), tw, tm, skip_tokens=1),
        "train_term_weights_dtype": lambda: LT.lexical_reps(tlg, tw.long(), tm, skip_tokens=1),
        "train_on_the_cpu": lambda: LT.lexical_reps(tlg, tw, tm, skip_tokens=1),
        "train_three_dimensional_sides_on_the_cpu": lambda: LT.lexical_reps(tlg, tw[..., None], tm[..., None], skip_tokens=1),
        # ---- dhr_amd.lexical_proj_train
        "ptrain_numpy_hidden": lambda: LPT.lexical_reps(np.zeros((2, 4, 16), np.float16), tW, tb, tw, tm),
        "ptrain_numpy_bias": lambda: LPT.lexical_reps(th, tW, np.zeros(8, f), tw, tm, skip_tokens=1),
        "ptrain_hidden_rank": lambda: LPT.lexical_reps(torch.zeros((2, 16)), tW, tb, tw, tm),
        "ptrain_weight_rank": lambda: LPT.lexical_reps(th, tW[0], tb, tw, tm, skip_tokens=1),
        "ptrain_weight_columns": lambda: LPT.lexical_reps(th, torch.zeros((8, 24), dtype=torch.float16), tb, tw, tm, skip_tokens=1),
        "ptrain_skip_negative": lambda: LPT.lexical_reps(th, tW, tb, tw, tm, skip_tokens=-1),
        "ptrain_all_skipped": lambda: LPT.lexical_reps(th, tW, tb, tw, tm, skip_tokens=4),
        "ptrain_no_tokens": lambda: LPT.lexical_reps(torch.zeros((2, 0, 16)), tW, tb, torch.zeros((2, 0)), torch.zeros((2, 0))),
        "ptrain_no_weight_rows": lambda: LPT.lexical_reps(th, torch.zeros((0, 16), dtype=torch.float16), None, tw, tm, skip_tokens=1),
        "ptrain_bias_shape": lambda: LPT.lexical_reps(th, tW, torch.zeros(7), tw, tm, skip_tokens=1),
        "ptrain_bias_rank": lambda: LPT.lexical_reps(th, tW, torch.zeros((8, 1)), tw, tm, skip_tokens=1),
        "ptrain_term_weights_shape": lambda: LPT.lexical_reps(th, tW, tb, torch.ones((2, 4)), tm, skip_tokens=1),
        "ptrain_mask_shape": lambda: LPT.lexical_reps(th, tW, tb, tw, torch.ones((3, 3)), skip_tokens=1),
        "ptrain_over_32767_tokens": lambda: LPT.lexical_reps(torch.zeros((1, 32768, 8), dtype=torch.float16), torch.zeros((8, 8), dtype=torch.float16), None,
                                                             torch.ones((1, 32768)), torch.ones((1, 32768))),
        "ptrain_hidden_dtype": lambda: LPT.lexical_reps(th.double(), tW, tb, tw, tm, skip_tokens=1),
        "ptrain_fp16_and_bf16_operands": lambda: LPT.lexical_reps(th, tW.to(bf), tb, tw, tm, skip_tokens=1),
        "ptrain_bias_dtype": lambda: LPT.lexical_reps(th, tW, tb.double(), tw, tm, skip_tokens=1),
        "ptrain_term_weights_dtype": lambda: LPT.lexical_reps(th, tW, tb, tw.long(), tm, skip_tokens=1),
        "ptrain_hidden_size_not_multiple_of_8": lambda: LPT.lexical_reps(torch.zeros((2, 4, 12), dtype=torch.float16), torch.zeros((8, 12), dtype=torch.float16), tb,
                                                                         tw, tm, skip_tokens=1),
        "ptrain_hidden_size_1032": lambda: LPT.lexical_reps(torch.zeros((2, 4, 1032), dtype=torch.float16), torch.zeros((8, 1032), dtype=torch.float16), tb, tw, tm,
                                                            skip_tokens=1),
        "ptrain_on_the_cpu": lambda: LPT.lexical_reps(th, tW, tb, tw, tm, skip_tokens=1),
        "ptrain_fp32_operands_on_the_cpu": lambda: LPT.lexical_reps(th.float(), tW.float(), None, tw, tm, skip_tokens=1),
    }
    return cases


def collect_python_exits():
    out = {}
    for name, call in _python_cases().items():
        try:
            call()
        except Exception as e:  # noqa: BLE001
            out[name] = [type(e).__name__, str(e)]
        else:
            out[name] = ["no exception", ""]
    return out


def collect_checks():
    """-> {"exits": {name: [status, last error text]}, "workspace": {...}, "python_exits": {name: [exception type, text]}}"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from dhr_amd import _lib
    lib = _lib.load()
    cases, keep = _check_cases(lib)
    exits = {}
    for name, call in cases.items():
        lib.dhr_merge_topk_host(0, 0, None, None, 0, None, None)          # a known error record in front of every case: one that succeeds leaves it
        exits[name] = [int(call()), lib.dhr_last_error().decode()]
    del keep
    return {"exits": exits, "workspace": _workspace_grid(lib), "python_exits": collect_python_exits()}


# ------------------------------------------------------------------------------------------------ what the heads compute (GPU)
def _bytes(torch, t):
    if isinstance(t, np.ndarray):
        return _digest(t)
    return _digest(t.detach().contiguous().cpu().view(torch.uint8).numpy())


def _shape_a(torch):
    rng = np.random.default_rng(SEED)
    x = (rng.standard_normal((B, L, V)) * 3.0).astype(np.float16)           # fp16 values: the fp32 and (rounded) bf16 inputs derive from them
    hid = (rng.standard_normal((B, L, H)) * 0.5).astype(np.float16)
    wgt = (rng.standard_normal((V, H)) * 0.5).astype(np.float16)
    bias = (rng.standard_normal(V) * 0.5).astype(np.float32)
    tw = (rng.standard_normal((B, T)) * 0.5 + 1.0).astype(np.float32)
    tw[1, 2] = -0.75                                                         # a masked token with a negative weight: its zero has a sign
    cls = rng.standard_normal((B, CLS)).astype(np.float32)
    g = rng.standard_normal((B, V)).astype(np.float32)
    return x, hid, wgt, bias, tw, cls, g


def _record_modes():
    """(name, mode arguments) of the record modes: raw, densify with both index dtypes, both aggregates; fp16 / fp32 records, with / without [CLS]"""
    yield "raw", None
    for rec in ("float16", "float32"):
        for cls in (0, CLS):
            for idx in ("uint8", "int16"):
                yield "densify_%s_%s_cls%d" % (idx, rec, cls), ("densify", rec, cls, idx)
            for full in (True, False):
                yield "agg_%s_%s_cls%d" % ("full" if full else "semi", rec, cls), ("agg", rec, cls, full)


def _records(torch, mod, args, like, cls_values, out):
    """every record mode of module `mod` (lexical or lexical_proj) on the inputs `args`; outputs where `like` lives, pre-filled, with spare columns"""
    from dhr_amd import _marshal as M
    for name, spec in _record_modes():
        if spec is None:
            out[name] = {"reps": _bytes(torch, mod.lexical_reps(*args))}
            continue
        kind, rec, cls, last = spec
        cols = DIMS if kind == "densify" else AGG_DIM

        def full(shape, dtype):
            a = M.empty(like, shape, dtype)
            a.fill(9) if M.is_np(a) else a.fill_(9)
            return a
        val = full((B, cols + cls + 3), rec)
        sem = None
        if cls:
            sem = cls_values.astype(rec) if M.is_np(like) else torch.from_numpy(cls_values.astype(rec)).to(like.device)
        if kind == "densify":
            idx = full((B, cols + 2), last)
            mod.densify_lexical_into(*args, val, idx, DIMS, REMOVE, semantic_reps=sem)
            out[name] = {"value": _bytes(torch, val), "index": _bytes(torch, idx)}
        else:
            mod.aggregate_lexical_into(*args, val, AGG_DIM, last, semantic_reps=sem)
            out[name] = {"value": _bytes(torch, val)}


def collect_lexical(torch, LX):
    x, _, _, _, tw, cls, _ = _shape_a(torch)
    dev = torch.device("cuda")
    w16, mask = torch.from_numpy(tw.astype(np.float16)).to(dev)[..., None], torch.from_numpy(MASK).to(dev)
    out = {}
    tx = torch.from_numpy(x).to(dev)
    inputs = {"device_float16": tx[:, 1:], "device_bfloat16": tx.to(torch.bfloat16)[:, 1:], "device_float32": tx.float()[:, 1:],
              "device_float16_packed": tx[:, 1:].contiguous()}
    for dt in (torch.float16, torch.bfloat16, torch.float32):               # the last-dimension view starts 4 elements in: its base is not 16-byte aligned
        wide = torch.zeros((B, T, V + 8), dtype=dt, device=dev)
        wide[:, :, 4:4 + V] = tx[:, 1:].to(dt)
        inputs["device_%s_offset4" % str(dt).replace("torch.", "")] = wide[:, :, 4:4 + V]
    for name, lg in inputs.items():
        rec = out[name] = {}
        _records(torch, LX, (lg, w16, mask), lg, cls, rec)
    for name, lg in (("numpy_float16", x[:, 1:]), ("numpy_float32", x.astype(np.float32)[:, 1:])):     # the staged path, from a [:, 1:] view
        rec = out[name] = {}
        _records(torch, LX, (lg, tw[..., None], MASK), lg, cls, rec)
    reps = LX.lexical_reps(inputs["device_float32"], w16, mask)
    for full in (True, False):                                              # dhr_aggregate on reps, from device and from host memory
        for dt in (torch.float16, torch.float32):
            src = reps.to(dt)
            name = "aggregate_%s_%s" % ("full" if full else "semi", str(dt).replace("torch.", ""))
            out[name] = {"device": _bytes(torch, LX.aggregate(src, AGG_DIM, full=full)), "numpy": _bytes(torch, LX.aggregate(src.cpu().numpy(), AGG_DIM, full=full))}
    return out


def collect_lexical_proj(torch, LP):
    _, hid, wgt, bias, tw, cls, _ = _shape_a(torch)
    dev = torch.device("cuda")
    w16, mask = torch.from_numpy(tw.astype(np.float16)).to(dev)[..., None], torch.from_numpy(MASK).to(dev)
    out = {}
    for dt, other in ((torch.float16, torch.bfloat16), (torch.bfloat16, torch.float16)):
        dn = str(dt).replace("torch.", "")
        th, tW = torch.from_numpy(hid).to(dev).to(dt), torch.from_numpy(wgt).to(dev).to(dt)
        tb = torch.from_numpy(bias).to(dev)
        for bname, b in (("none", None), ("float32", tb), ("same", tb.to(dt)), ("other", tb.to(other))):      # "other" next to fp16 operands: widened to fp32
            rec = out["%s_bias_%s" % (dn, bname)] = {}
            _records(torch, LP, (th[:, 1:], tW, b, w16, mask), th, cls, rec)
        wide_h = torch.zeros((B, T, H + 8), dtype=dt, device=dev)
        wide_h[:, :, 4:4 + H] = th[:, 1:]
        wide_w = torch.zeros((V, H + 8), dtype=dt, device=dev)
        wide_w[:, 4:4 + H] = tW
        rec = out["%s_offset4" % dn] = {}                                    # vec_h = vec_w = 0
        _records(torch, LP, (wide_h[:, :, 4:4 + H], wide_w[:, 4:4 + H], tb, w16, mask), th, cls, rec)
        wide_w2 = torch.zeros((V, H + 8), dtype=dt, device=dev)
        wide_w2[:, :H] = tW
        rec = out["%s_weight_row_stride" % dn] = {}
        _records(torch, LP, (th[:, 1:], wide_w2[:, :H], tb, w16, mask), th, cls, rec)
    return out


def _grads(torch, reps, tok, leaves, upstream):
    """digests of the forward and of every gradient after reps.sum().backward() and after a seeded random upstream gradient"""
    rec = {"reps": _bytes(torch, reps), "tok": _bytes(torch, tok)}
    live = {n: t for n, t in leaves.items() if t is not None and t.requires_grad}
    for tag, g in (("sum", None), ("random", upstream)):
        for t in live.values():
            t.grad = None
        if not live:
            continue
        (reps.sum() if g is None else (reps * g).sum()).backward(retain_graph=True)
        for n, t in live.items():
            rec["grad_%s_after_%s" % (n, tag)] = _bytes(torch, t.grad)
    return rec


def collect_lexical_train(torch, LT):
    x, _, _, _, tw, _, g = _shape_a(torch)
    dev = torch.device("cuda")
    mask, up = torch.from_numpy(MASK).to(dev), torch.from_numpy(g).to(dev)
    out = {}
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        dn = str(dt).replace("torch.", "")
        for variant in ("whole_skip1", "view_skip0", "weights_3d", "detached_logits", "detached_weights"):
            tx = torch.from_numpy(x).to(dev).to(dt).requires_grad_(variant != "detached_logits")
            w = torch.from_numpy(tw).to(dev).to(torch.float16 if dt == torch.float16 else torch.float32)
            w = (w[..., None] if variant == "weights_3d" else w).clone().requires_grad_(variant != "detached_weights")
            if variant == "view_skip0":
                reps, tok = LT.lexical_reps(tx[:, 1:], w, mask, skip_tokens=0, return_tokens=True)
            else:
                reps, tok = LT.lexical_reps(tx, w, mask, skip_tokens=1, return_tokens=True)
            out["%s_%s" % (dn, variant)] = _grads(torch, reps, tok, {"logits": tx, "term_weights": w}, up)
    return out


def _proj_train_case(torch, LPT, dt, variant, hid, wgt, bias, tw, mask, up, skip=1):
    dev = torch.device("cuda")
    frozen = variant == "frozen_projector"
    th = torch.from_numpy(hid).to(dev).to(dt).requires_grad_(variant != "detached_hidden")
    tW = torch.from_numpy(wgt).to(dev).to(dt).requires_grad_(not frozen)
    tb = None if variant == "no_bias" else torch.from_numpy(bias).to(dev).to(torch.float32 if variant == "bias_float32" else dt).requires_grad_(not frozen)
    w = torch.from_numpy(tw).to(dev)
    w = (w[..., None] if variant == "weights_3d" else w).clone().requires_grad_(True)
    if variant == "view_skip0":
        reps, tok = LPT.lexical_reps(th[:, skip:], tW, tb, w, mask, skip_tokens=0, return_tokens=True)
    else:
        reps, tok = LPT.lexical_reps(th, tW, tb, w, mask, skip_tokens=skip, return_tokens=True)
    return _grads(torch, reps, tok, {"hidden": th, "weight": tW, "bias": tb, "term_weights": w}, up)


def collect_lexical_proj_train(torch, LPT):
    _, hid, wgt, bias, tw, _, g = _shape_a(torch)
    dev = torch.device("cuda")
    mask, up = torch.from_numpy(MASK).to(dev), torch.from_numpy(g).to(dev)
    out = {}
    for dt in (torch.float16, torch.bfloat16):
        dn = str(dt).replace("torch.", "")
        for variant in ("whole_skip1", "view_skip0", "weights_3d", "frozen_projector", "detached_hidden", "no_bias", "bias_float32"):
            out["%s_%s" % (dn, variant)] = _proj_train_case(torch, LPT, dt, variant, hid, wgt, bias, tw, mask, up)
    # shape B: one passage, two tokens, one vocabulary tile; H just above the one-slab limit of the gradient passes (12 chunks of 64) and the widest H
    rng = np.random.default_rng(SEED + 1)
    for hb in (12 * 64 + 8, 1024):
        hid_b, wgt_b = (rng.standard_normal((1, 2, hb)) * 0.25).astype(np.float16), (rng.standard_normal((256, hb)) * 0.25).astype(np.float16)
        bias_b, tw_b = (rng.standard_normal(256) * 0.5).astype(np.float32), np.array([[1.25, 0.5]], np.float32)
        mask_b, up_b = torch.ones((1, 2), dtype=torch.long, device=dev), torch.from_numpy(rng.standard_normal((1, 256)).astype(np.float32)).to(dev)
        for dt in (torch.float16, torch.bfloat16):
            out["shape_b_h%d_%s" % (hb, str(dt).replace("torch.", ""))] = _proj_train_case(torch, LPT, dt, "whole_skip0", hid_b, wgt_b, bias_b, tw_b, mask_b, up_b,
                                                                                          skip=0)
    return out


def staged_second_block(torch, LX):
    """shape C: fp32 numpy logits [18, 128, 30522] -- 17 rows fit the 256 MiB staging block, so the staged loop of dhr_lexical_head runs a second
    block of one row.  -> (digest of the raw reps from host memory, digest of the same call on device memory)"""
    rng = np.random.default_rng(SEED + 2)
    lg = rng.standard_normal((18, 128, 30522), dtype=np.float32)
    w = rng.standard_normal((18, 128), dtype=np.float32)
    m = (rng.random((18, 128)) < 0.9).astype(np.int64)
    m[:, 0] = 1
    host = LX.lexical_reps(lg, w, m)
    dev = LX.lexical_reps(torch.from_numpy(lg).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(m).cuda())
    return _digest(host), _bytes(torch, dev)


def collect_gpu():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import torch
    from dhr_amd import lexical as LX, lexical_proj as LP, lexical_proj_train as LPT, lexical_train as LT
    out = {"lexical": collect_lexical(torch, LX), "lexical_proj": collect_lexical_proj(torch, LP), "lexical_train": collect_lexical_train(torch, LT),
           "lexical_proj_train": collect_lexical_proj_train(torch, LPT)}
    host, dev = staged_second_block(torch, LX)
    out["staged_second_block"] = {"host": host, "device": dev}
    return out


def leaves(d, prefix=""):
    """{dotted path: value} of a nested dict"""
    out = {}
    for key, v in d.items():
        if isinstance(v, dict):
            out.update(leaves(v, prefix + key + "."))
        else:
            out[prefix + key] = v
    return out


def _write(path, obj):
    with open(path, "w") as f:
        json.dump(obj, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


def main():
    argv = sys.argv[1:]
    path = argv[argv.index("--out") + 1] if "--out" in argv else None
    if "--checks" in argv:
        _write(path or PATH_CHECKS, collect_checks())
    if "--gpu" in argv:
        got = collect_gpu()
        if "--verify" not in argv:
            _write(path or PATH_GPU, got)
            return 0
        with open(path or PATH_GPU) as f:
            before = leaves(json.load(f))
        now = leaves(got)
        differ = sorted(p for p in set(before) | set(now) if before.get(p) != now.get(p))
        print("%d fields, %d differ from the file%s" % (len(now), len(differ), ":" if differ else ""), *differ, sep="\n  ")
        return 1 if differ else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
