// The workspace of the lexical heads with the vocabulary projection fused in (lexical_proj.hip: encoding, lexical_proj_train.hip: training), as
// plain host arithmetic: no HIP include, so tests/lexical_proj_layout_check.cpp compiles this header alone.  Both heads run the same forward
// (lexical_proj_common.h) on the same first seven sections; the encoding layout appends the fp32 reps that its record epilogues read, the
// training layout what the backward keeps.  Every section starts at a multiple of 256 bytes; its size is in the comments of ProjArgs.
#pragma once
#include <algorithm>
#include <cstdint>

namespace {

constexpr int TM = 64;                 // token rows of a tile
constexpr int TN = 256;                // vocabulary columns of a tile: 64 per wave
constexpr int MAX_SPLIT = 16;          // shares of the vocabulary in the statistics pass, and in pass 2 of the backward
constexpr int FILL_WGS = 1024;         // workgroups the statistics pass wants
constexpr int SPLIT_WGS = 256;         // pass 2 splits the vocabulary into shares where the worst-case list has fewer 64-row tiles than half of this

inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

// 64-row tiles of the worst-case list of BT token rows
inline int64_t proj_m_tiles(int64_t BT) { return std::max<int64_t>(1, (BT + TM - 1) / TM); }
// shares of the vocabulary where `per_tile` workgroups are wanted per 64-row tile: at least 1, at most MAX_SPLIT and the vocabulary tiles
inline int proj_split(int n_ntiles, int64_t per_tile) {
  return (int)std::min<int64_t>(std::min<int64_t>(MAX_SPLIT, n_ntiles), std::max<int64_t>(1, per_tile));
}
// ... in the statistics pass: enough workgroups to fill the chip when there are few token rows
inline int proj_stats_split(int64_t BT, int n_ntiles) { return proj_split(n_ntiles, (FILL_WGS + proj_m_tiles(BT) - 1) / proj_m_tiles(BT)); }

// what the forward of both heads keeps: byte offsets of the sections, `end` the first byte behind them
struct ProjLayout {
  int64_t hdr, cnt, start, tmask, rows, stats, part, end;
  int n_split, n_ntiles;
};

inline ProjLayout proj_layout(int64_t B, int T, int V) {
  ProjLayout l{};
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
  l.end = at;
  return l;
}

// encoding: + the fp32 reps [B, V], unless they are the output itself (raw mode)
struct ProjEncodeLayout : ProjLayout {
  int64_t reps, total;
};

inline ProjEncodeLayout proj_encode_layout(int64_t B, int T, int V, bool with_reps) {
  ProjEncodeLayout l{proj_layout(B, T, V), 0, 0};
  l.reps = l.end;
  l.total = with_reps ? align256(l.reps + 4 * B * V) : l.reps;
  return l;
}

// training: + D [B * T] fp32 and, where pass 2 of the backward splits the vocabulary, its partial sums [grad_split][B * T][H] fp32
struct ProjTrainLayout : ProjLayout {
  int64_t D, partial, total;
  int grad_split;
};

inline ProjTrainLayout proj_train_layout(int64_t B, int T, int V, int H) {
  ProjTrainLayout l{proj_layout(B, T, V), 0, 0, 0, 0};
  const int64_t BT = B * T;
  l.grad_split = proj_split(l.n_ntiles, SPLIT_WGS / proj_m_tiles(BT));
  l.D = l.end;
  l.partial = align256(l.D + 4 * BT);
  l.total = l.grad_split > 1 ? align256(l.partial + 4 * BT * H * l.grad_split) : l.partial;
  return l;
}

}  // namespace
