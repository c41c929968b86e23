// Where the validated dtype codes of the C ABI (host_stage.h: val_ok, val_ok_bf16, idx_ok) become C++ types, once, for the launchers of the op
// translation units.  Each dispatcher takes a run-time code and a generic lambda, calls the lambda exactly once with the tag (TypeTag<T>) or the
// constant (std::true_type, std::integral_constant<int, N>) of the selected arm and returns what the lambda returns:
//
//     with_value_type(grad_dtype, [&](auto t) { with_flag(vec, [&](auto v) {
//       using T = typename decltype(t)::type;
//       hipLaunchKernelGGL((kernel<T, decltype(v)::value>), grid, block, 0, s, (const T*)grad, ...);
//     }); });
//
// Plain if-chains over templates: no virtual calls, no std::function, no tables; inlined, the host code is the ladder one would write by hand.
// A code outside a dispatcher's list runs no arm: it throws std::logic_error, which the exception barrier of the C ABI (abi_guard.h) turns
// into DHR_ERR_INTERNAL.  Every entry point rejects such a code with its own message before it launches, so no caller gets there.
// Host-only, no HIP header: tests/op_dispatch_check.cpp compiles it as plain C++17.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <type_traits>
#include <utility>

#include "../../include/dhr_hip.h"

template <class T> struct TypeTag { using type = T; };

// f(TypeTag<the i-th of T, Ts...>{}): the primitive
template <class T, class... Ts, class F>
auto pick_type(int i, F&& f) -> decltype(f(TypeTag<T>{})) {
  if (i == 0) return f(TypeTag<T>{});
  if constexpr (sizeof...(Ts) > 0) return pick_type<Ts...>(i - 1, std::forward<F>(f));
  else throw std::logic_error("op dispatch: a dtype code outside the list");
}

// (the arms stand in the order in which the launchers have always named them, fp32 first: it is the order of the kernels in the code object)
template <class F> auto with_value_type(int val_dtype, F&& f) {
  return pick_type<float, _Float16>(val_dtype == DHR_VAL_F32 ? 0 : val_dtype == DHR_VAL_F16 ? 1 : -1, std::forward<F>(f));
}
// the lexical heads alone (val_ok_bf16)
template <class F> auto with_value_type_bf16(int val_dtype, F&& f) {
  return pick_type<float, __bf16, _Float16>(val_dtype == DHR_VAL_F32 ? 0 : val_dtype == DHR_VAL_BF16 ? 1 : val_dtype == DHR_VAL_F16 ? 2 : -1, std::forward<F>(f));
}
// the operands of the projection heads: the two MFMA input types, never fp32
template <class F> auto with_half_type(int val_dtype, F&& f) {
  return pick_type<__bf16, _Float16>(val_dtype == DHR_VAL_BF16 ? 0 : val_dtype == DHR_VAL_F16 ? 1 : -1, std::forward<F>(f));
}
template <class F> auto with_index_type(int idx_dtype, F&& f) {
  return pick_type<uint8_t, int8_t, int16_t>(idx_dtype == DHR_IDX_U8 ? 0 : idx_dtype == DHR_IDX_I8 ? 1 : idx_dtype == DHR_IDX_I16 ? 2 : -1, std::forward<F>(f));
}
template <class F> auto with_id_type(int id_bytes, F&& f) {
  return pick_type<int64_t, int32_t>(id_bytes == 8 ? 0 : id_bytes == 4 ? 1 : -1, std::forward<F>(f));
}

template <class F> auto with_flag(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

// f(std::integral_constant<int, n>{}) for n one of N, Ns...
template <int N, int... Ns, class F>
auto with_int(int n, F&& f) -> decltype(f(std::integral_constant<int, N>{})) {
  if (n == N) return f(std::integral_constant<int, N>{});
  if constexpr (sizeof...(Ns) > 0) return with_int<Ns...>(n, std::forward<F>(f));
  else throw std::logic_error("op dispatch: a constant outside the list");
}
