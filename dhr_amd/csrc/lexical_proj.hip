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
#include "host_stage.h"
#include "lexical_proj_common.h"

namespace {

struct Layout {
  int64_t hdr, cnt, start, tmask, rows, stats, part, reps, total;
  int n_split, n_ntiles;
};

Layout layout(int64_t B, int T, int V, int mode) {
  Layout l{};
  const int64_t BT = B * T;
  l.n_ntiles = (V + TN - 1) / TN;
  l.n_split = proj_stats_split(BT, l.n_ntiles);
  int64_t at = 0;
  l.hdr = at; at += 256;
  l.cnt = at; at = align256(at + 4 * B);
  l.start = at; at = align256(at + 4 * (B + 1));
  l.tmask = at; at = align256(at + 4 * B);
  l.rows = at; at = align256(at + 4 * BT);
  l.stats = at; at = align256(at + 16 * BT);
  l.part = at; at = align256(at + 8 * BT * l.n_split);
  l.reps = at;
  if (mode != MODE_RAW) at = align256(at + 4 * B * V);
  l.total = at;
  return l;
}

}  // namespace

extern "C" int64_t dhr_lexical_proj_workspace(int64_t batch, int32_t n_tokens, int32_t vocab, int32_t mode) try {
  if (batch < 0 || n_tokens <= 0 || vocab <= 0 || batch * n_tokens > ((int64_t)1 << 31) - 1) return 0;
  return layout(batch, n_tokens, vocab, mode).total;
} DHR_CATCH_VALUE(0)

extern "C" int dhr_lexical_proj_head(int32_t device, int32_t mem_kind, int32_t mode, const void* hidden, int32_t value_dtype, int64_t batch,
                                     int32_t n_tokens, int32_t hidden_dim, int64_t ld_batch, int64_t ld_token, const void* weight, int32_t vocab,
                                     int64_t ld_weight, const void* bias, int32_t bias_dtype, const float* term_weights, int64_t ld_weights,
                                     const float* mask, int64_t ld_mask, int32_t dims, int32_t remove_dims, void* out_value, int32_t out_value_dtype,
                                     int64_t ld_value, void* out_index, int32_t index_dtype, int64_t ld_index, const void* cls, int32_t cls_dtype,
                                     int64_t ld_cls, int32_t cls_dim, void* workspace, int64_t workspace_bytes, void* stream) try {
  dhr::alloc_checkpoint();
  if (!hidden || !weight || !term_weights || !mask || !out_value) return set_error(DHR_ERR_INVALID, "null pointer");
  if (mem_kind != DHR_MEM_DEVICE) return set_error(DHR_ERR_INVALID, "lexical projection head: device memory only");
  if (!val_ok_bf16(value_dtype) || !val_ok(out_value_dtype) || (bias && !val_ok_bf16(bias_dtype))) return set_error(DHR_ERR_INVALID, "bad value dtype");
  if (value_dtype == DHR_VAL_F32) return set_error(DHR_ERR_UNSUPPORTED, "lexical projection head: hidden states and weight must be fp16 or bf16");
  if (bias && bias_dtype == DHR_VAL_BF16 && value_dtype == DHR_VAL_F16)
    return set_error(DHR_ERR_UNSUPPORTED, "lexical projection head: a bf16 bias needs bf16 hidden states and weight (the fp16 kernels read fp32 or fp16)");
  if (batch < 0 || n_tokens <= 0 || vocab <= 0 || hidden_dim <= 0 || ld_token < hidden_dim ||
      ld_batch < (int64_t)(n_tokens - 1) * ld_token + hidden_dim || ld_weight < hidden_dim || ld_weights < n_tokens || ld_mask < n_tokens ||
      cls_dim < 0 || workspace_bytes < 0 || (int64_t)batch * n_tokens > ((int64_t)1 << 31) - 1)
    return set_error(DHR_ERR_INVALID, "bad sizes / strides");
  if (hidden_dim % 8) return set_error(DHR_ERR_INVALID, "the hidden size must be a multiple of 8");
  Geometry geo;
  int rc = geometry(mode, vocab, dims, remove_dims, geo);
  if (rc) return rc;
  if (ld_value < (int64_t)geo.out_cols + cls_dim) return set_error(DHR_ERR_INVALID, "ld_value is smaller than the record's columns");
  if (cls_dim > 0 && (!cls || !val_ok(cls_dtype) || ld_cls < cls_dim)) return set_error(DHR_ERR_INVALID, "bad cls reps");
  if (mode == MODE_DENSIFY) {
    if (!out_index) return set_error(DHR_ERR_INVALID, "null index pointer");
    if (index_dtype != DHR_IDX_U8 && index_dtype != DHR_IDX_I16) return set_error(DHR_ERR_INVALID, "index dtype must be uint8 or int16");
    if (index_dtype == DHR_IDX_U8 && geo.n_groups > 256) return set_error(DHR_ERR_UNSUPPORTED, "more than 256 groups need the int16 index dtype");
    if (ld_index < geo.out_cols) return set_error(DHR_ERR_INVALID, "ld_index < dims");
  }
  if (mode == MODE_RAW && out_value_dtype != DHR_VAL_F32) return set_error(DHR_ERR_UNSUPPORTED, "lexical projection head: raw reps are fp32");
  if (batch == 0) return DHR_OK;
  const Layout l = layout(batch, n_tokens, vocab, mode);
  if (!workspace || workspace_bytes < l.total)
    return set_error(DHR_ERR_INVALID, "workspace is smaller than dhr_lexical_proj_workspace (" + std::to_string(l.total) + " bytes)");
  if ((uintptr_t)workspace % 16) return set_error(DHR_ERR_INVALID, "workspace must be aligned to 16 bytes");
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  ProjArgs a{};
  a.hid = (const _Float16*)hidden; a.ld_hb = ld_batch; a.ld_ht = ld_token;
  a.wgt = (const _Float16*)weight; a.ld_w = ld_weight;
  a.bias = bias; dtype_flags(bias_dtype, a.bias_f32, a.bias_f16);
  a.tw = term_weights; a.ld_tw = ld_weights; a.mask = mask; a.ld_mask = ld_mask;
  a.B = batch; a.T = n_tokens; a.H = hidden_dim; a.V = vocab;
  a.vec_h = (uintptr_t)hidden % 16 == 0 && ld_batch % 8 == 0 && ld_token % 8 == 0;
  a.vec_w = (uintptr_t)weight % 16 == 0 && ld_weight % 8 == 0;
  a.n_split = l.n_split; a.n_ntiles = l.n_ntiles;
  a.group = (int)std::max<int64_t>((GROUP_ROWS + n_tokens - 1) / n_tokens, (batch + 65534) / 65535);
  a.hdr = (int*)(ws + l.hdr); a.cnt = (int*)(ws + l.cnt); a.start = (int*)(ws + l.start); a.tmask = (int*)(ws + l.tmask);
  a.rows = (int*)(ws + l.rows); a.stats = (float4*)(ws + l.stats); a.part = (float2*)(ws + l.part);
  const bool direct = mode == MODE_RAW;                  // fp32 reps are the output itself
  a.reps = direct ? (float*)out_value : (float*)(ws + l.reps);
  a.ld_reps = direct ? ld_value : vocab;
  launch_forward<false>(value_dtype, a, s);
  HIP_TRY(hipGetLastError());
  HIP_TRY(dhr::lexical_record_from_reps(direct ? nullptr : a.reps, vocab, mode, batch, vocab, geo.out_cols, geo.W, geo.n_groups, geo.remove, out_value,
                                        out_value_dtype == DHR_VAL_F32, ld_value, out_index, index_dtype == DHR_IDX_I16, ld_index, cls,
                                        cls_dtype == DHR_VAL_F32, ld_cls, cls_dim, s));
  return DHR_OK;
} DHR_CATCH_STATUS
