// Host code shared by the op translation units (gip_train, maxsim, train_loss, lexical*, aggretriever_train, densify in api.hip): the dtype
// checks of the C ABI and the staging of host arrays through the device.  A staged call owns its device copies in DevMem objects, enqueues
// every copy on the caller's stream and synchronises that stream itself before it returns.  The step from a code that passed these checks to a
// C++ type is op_dispatch.h (with_value_type, with_index_type, ...), which the launchers that pick a kernel instance include next to this header.
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
