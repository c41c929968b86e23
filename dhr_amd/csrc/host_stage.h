// Host code shared by the translation units that take arrays from host or device memory (the op files gip_train, maxsim, train_loss and
// aggretriever_train; the lexical heads, through lexical_common.h -- dhr_lexical_head and dhr_aggregate stage host arrays with it; the entry points
// of api.hip; the PQ handle of pq_adc.hip): the dtype checks of the C ABI and the ONE vocabulary for staging host arrays through the device.  A staged call owns its device copies in DevMem objects, enqueues every copy on the caller's stream and
// synchronises that stream itself before it returns.  Matrices with a row stride go through the 2-D forms, contiguous arrays through the flat
// ones; operand_in / operand_out give "the device view of an operand" (the pointer itself for device memory, else a staged copy), emit_topk hands
// a sorted top-k out.  The step from a code that passed these checks to a C++ type is op_dispatch.h (with_value_type, with_index_type, ...),
// which the launchers that pick a kernel instance include next to this header.
#pragma once
#include "dhr_state.h"

static inline int val_ok(int dt) { return dt == DHR_VAL_F16 || dt == DHR_VAL_F32; }
// the lexical heads alone: their logits / operands, the projection's bias and the gradients of their backward calls may also be bf16
static inline int val_ok_bf16(int dt) { return val_ok(dt) || dt == DHR_VAL_BF16; }
static inline int idx_ok(int dt) { return dt == DHR_IDX_U8 || dt == DHR_IDX_I8 || dt == DHR_IDX_I16; }
static inline int val_esize(int dt) { return dt == DHR_VAL_F32 ? 4 : 2; }

// device scratch of a call, released when m goes out of scope (zero bytes still give a pointer)
static inline hipError_t dev_alloc(DevMem& m, int64_t bytes) { return hipMalloc(&m.p, (size_t)std::max<int64_t>(1, bytes)); }

// a host matrix [rows, cols] of es-byte elements with row stride ld (in elements) -> the packed device buffer dev (row stride cols), and back
static inline hipError_t copy_in(void* dev, const void* host, int64_t ld, int64_t rows, int64_t cols, int es, hipStream_t s) {
  if (rows == 0 || cols == 0) return hipSuccess;
  return hipMemcpy2DAsync(dev, (size_t)cols * es, host, (size_t)ld * es, (size_t)cols * es, (size_t)rows, hipMemcpyHostToDevice, s);
}
static inline hipError_t stage_out(void* host, int64_t ld, const void* dev, int64_t rows, int64_t cols, int es, hipStream_t s) {
  if (rows == 0 || cols == 0) return hipSuccess;
  return hipMemcpy2DAsync(host, (size_t)ld * es, dev, (size_t)cols * es, (size_t)cols * es, (size_t)rows, hipMemcpyDeviceToHost, s);
}
// allocates the packed device copy, then copy_in
static inline hipError_t stage_in(DevMem& m, const void* host, int64_t ld, int64_t rows, int64_t cols, int es, hipStream_t s) {
  const hipError_t e = dev_alloc(m, rows * cols * es);
  return e != hipSuccess ? e : copy_in(m.p, host, ld, rows, cols, es, s);
}
// ... and the same three for a contiguous array of `bytes` bytes
static inline hipError_t copy_in(void* dev, const void* host, size_t bytes, hipStream_t s) {
  return bytes ? hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
}
static inline hipError_t stage_out(void* host, const void* dev, size_t bytes, hipStream_t s) {
  return bytes ? hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
}
static inline hipError_t stage_in(DevMem& m, const void* host, size_t bytes, hipStream_t s) {
  const hipError_t e = dev_alloc(m, (int64_t)bytes);
  return e != hipSuccess ? e : copy_in(m.p, host, bytes, s);
}

// The device view of a contiguous operand that a call takes from host or device memory: the pointer itself for device memory, else a staged
// copy that m owns.  operand_in copies the host array in; operand_out only allocates, and operand_back copies out what operand_out staged
// (nothing for device memory).
template <typename T>
hipError_t operand_in(DevMem& m, int mem_kind, const T* a, size_t bytes, hipStream_t s, const T*& view) {
  view = a;
  if (mem_kind != DHR_MEM_HOST) return hipSuccess;
  const hipError_t e = stage_in(m, a, bytes, s);
  view = (const T*)m.p;
  return e;
}
template <typename T>
hipError_t operand_out(DevMem& m, int mem_kind, T* a, size_t bytes, T*& view) {
  view = a;
  if (mem_kind != DHR_MEM_HOST) return hipSuccess;
  const hipError_t e = dev_alloc(m, (int64_t)bytes);
  view = (T*)m.p;
  return e;
}
static inline hipError_t operand_back(const DevMem& m, void* a, size_t bytes, hipStream_t s) { return m.p ? stage_out(a, m.p, bytes, s) : hipSuccess; }

// The sorted top-k keys of Q queries (key rows kp apart) -> the caller's score / row arrays [Q, k].  Host arrays go through `stage`: device
// scratch of Q * k * 12 bytes that the caller owns.  The copies are enqueued.
static inline int emit_topk(const uint64_t* keys, int kp, int Q, int k, int64_t row_offset, float* out_scores, int64_t* out_rows, int out_mem_kind,
                            void* stage, hipStream_t s) {
  const bool host = out_mem_kind == DHR_MEM_HOST;
  int64_t* d_rows = host ? (int64_t*)stage : out_rows;
  float* d_scores = host ? (float*)((char*)stage + (size_t)Q * k * 8) : out_scores;
  HIP_TRY(launch_emit(keys, kp, Q, k, row_offset, d_scores, d_rows, s));
  if (host) {
    HIP_TRY(stage_out(out_rows, d_rows, (size_t)Q * k * 8, s));
    HIP_TRY(stage_out(out_scores, d_scores, (size_t)Q * k * 4, s));
  }
  return DHR_OK;
}
