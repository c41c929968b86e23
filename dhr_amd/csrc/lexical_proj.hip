// The lexical head of an ENCODING run with the vocabulary projection fused in.  The reference makes the MLM logits [B, T, V] with the last
// linear layer of the MLM head and reads them back in encode_passage / encode_query (tevatron/DHR/modeling.py:291-300,322-331,
// tevatron/Aggretriever/modeling.py:274-278); dhr_lexical_head (lexical.hip) starts from that tensor.  Here the op starts from the projector's
// input: hidden [B, T, H] and weight [V, H], both fp16 or both bf16, and bias [V], and the logits
//   x[b][t][v] = sum_k hidden[b][t][k] * weight[v][k] + bias[v]          (fp32 products and sums, never rounded to 16 bits)
// exist only as MFMA accumulators.  Masked tokens are compacted away first, so they are never multiplied:
//   proj_count / proj_scan / proj_fill   the list of unmasked token rows in (passage, token) order, the first row of every passage in it, and
//                                        the first masked token of every passage
//   proj_stats_kernel     GEMM pass 1 over (64 token rows) x (a share of the vocabulary, 256 columns at a time), tokens on the lanes of
//                         v_mfma_f32_32x32x16_f16 (_bf16 for bf16 operands): a lane keeps the running (max, sum exp) of its token across the
//                         tiles and the workgroup writes one partial per (token, share)
//   proj_combine_kernel   the partials of a token in share order (fp64) -> (max, sum, w, mask) per row, the statistics lexical_fold_kernel reads
//   proj_fold_kernel      GEMM pass 2: a workgroup owns (256 vocabulary columns, a group of passages) and walks the group's token rows 64 at a
//                         time, in order, tokens in the accumulator registers.  The lane halves swap one of their two column tiles, so a lane
//                         holds all 64 rows of ONE column and folds expf(x - max) / sum, (p * w) * mask with strict > in token order; a passage
//                         may begin and end anywhere in a tile and span tiles (the running maximum lives in a register), and its row of the
//                         [B, V] fp32 reps is written when its last token has been folded.  No atomics.
// A masked token contributes (p * w) * 0, a zero with the sign of w, and zeros compare equal: only the first masked token of a passage can
// matter, and it is folded in at its place in token order (before the first unmasked token that follows it, or after the passage's last).
// The record epilogues (raw / densify / aggregate, [CLS] columns) are those of lexical.hip on the fp32 reps (lexical_record_from_reps).
// Every reduction has a fixed order: two calls on the same arguments are bit-identical.  NaN / inf inputs are out of scope.
#include "lexical_proj_common.h"

extern "C" int64_t dhr_lexical_proj_workspace(int64_t batch, int32_t n_tokens, int32_t vocab, int32_t mode) try {
  if (batch < 0 || n_tokens <= 0 || vocab <= 0 || batch * n_tokens > ((int64_t)1 << 31) - 1) return 0;
  return proj_encode_layout(batch, n_tokens, vocab, mode != MODE_RAW).total;
} DHR_CATCH_VALUE(0)

extern "C" int dhr_lexical_proj_head(int32_t device, int32_t mem_kind, int32_t mode, const void* hidden, int32_t value_dtype, int64_t batch,
                                     int32_t n_tokens, int32_t hidden_dim, int64_t ld_batch, int64_t ld_token, const void* weight, int32_t vocab,
                                     int64_t ld_weight, const void* bias, int32_t bias_dtype, const float* term_weights, int64_t ld_weights,
                                     const float* mask, int64_t ld_mask, int32_t dims, int32_t remove_dims, void* out_value, int32_t out_value_dtype,
                                     int64_t ld_value, void* out_index, int32_t index_dtype, int64_t ld_index, const void* cls, int32_t cls_dtype,
                                     int64_t ld_cls, int32_t cls_dim, void* workspace, int64_t workspace_bytes, void* stream) try {
  dhr::alloc_checkpoint();
  if (!out_value) return set_error(DHR_ERR_INVALID, "null pointer");
  const ProjOperands o{mem_kind, hidden, value_dtype, batch, n_tokens, 0, hidden_dim, ld_batch, ld_token, weight, vocab, ld_weight, bias, bias_dtype,
                       term_weights, ld_weights, mask, ld_mask, workspace, workspace_bytes};
  int rc = check_operands("lexical projection head", false, o, val_ok(out_value_dtype), cls_dim >= 0);
  if (rc) return rc;
  Geometry geo;
  rc = check_record(mode, vocab, dims, remove_dims, ld_value, out_index, index_dtype, ld_index, cls, cls_dtype, ld_cls, cls_dim, geo);
  if (rc) return rc;
  const bool direct = mode == MODE_RAW;                  // fp32 reps are the output itself
  if (direct && out_value_dtype != DHR_VAL_F32) return set_error(DHR_ERR_UNSUPPORTED, "lexical projection head: raw reps are fp32");
  if (batch == 0) return DHR_OK;
  const ProjEncodeLayout l = proj_encode_layout(batch, n_tokens, vocab, !direct);
  rc = check_workspace("dhr_lexical_proj_workspace", l.total, o);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  ProjArgs a = proj_args(l, o);
  a.reps = direct ? (float*)out_value : (float*)((char*)workspace + l.reps);
  a.ld_reps = direct ? ld_value : vocab;
  launch_forward<false>(value_dtype, a, s);
  HIP_TRY(hipGetLastError());
  HIP_TRY(dhr::lexical_record_from_reps(direct ? nullptr : a.reps, vocab, mode, batch, vocab, geo.out_cols, geo.W, geo.n_groups, geo.remove, out_value,
                                        out_value_dtype == DHR_VAL_F32, ld_value, out_index, index_dtype == DHR_IDX_I16, ld_index, cls,
                                        cls_dtype == DHR_VAL_F32, ld_cls, cls_dim, s));
  return DHR_OK;
} DHR_CATCH_STATUS
