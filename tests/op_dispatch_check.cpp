// The dispatchers of dhr_amd/csrc/op_dispatch.h on the CPU: for every dispatcher and every code in its list the lambda runs exactly once, with
// the expected tag or constant, and its return value comes back; nested dispatchers visit the full product; a code outside the list throws and
// runs no arm.  Built and run by tests/test_op_dispatch.py as host C++ with -fsanitize=address,undefined; includes nothing of the library but
// that header.
#include "op_dispatch.h"

#include <cstdio>
#include <cstdlib>

static long n_arms = 0;
#define CHECK(cond)                                                            \
  do {                                                                         \
    if (!(cond)) {                                                             \
      std::fprintf(stderr, "FAILED %s (line %d, %s)\n", #cond, __LINE__, what); \
      std::exit(1);                                                            \
    }                                                                          \
  } while (0)

// dispatch(f) calls one dispatcher with one code: f must run once, with a Want, and what it returns must come back
template <class Want, class Dispatch>
static void expect(const char* what, Dispatch&& dispatch) {
  int runs = 0, hits = 0;
  const int token = 1000 + (int)n_arms;
  const int got = dispatch([&](auto arm) -> int {
    ++runs;
    hits += std::is_same<decltype(arm), Want>::value;
    return token;
  });
  CHECK(runs == 1);
  CHECK(hits == 1);
  CHECK(got == token);
  ++n_arms;
}

template <class Dispatch>
static void expect_miss(const char* what, Dispatch&& dispatch) {
  int runs = 0;
  bool threw = false;
  try {
    dispatch([&](auto) -> int { ++runs; return 0; });
  } catch (const std::logic_error&) {
    threw = true;
  }
  CHECK(threw);
  CHECK(runs == 0);
}

template <int N> using Int = std::integral_constant<int, N>;

template <class T> constexpr int val_code() {
  return std::is_same<T, float>::value ? DHR_VAL_F32 : std::is_same<T, _Float16>::value ? DHR_VAL_F16 : std::is_same<T, __bf16>::value ? DHR_VAL_BF16 : -1;
}
template <class T> constexpr int idx_code() {
  return std::is_same<T, uint8_t>::value ? DHR_IDX_U8 : std::is_same<T, int8_t>::value ? DHR_IDX_I8 : std::is_same<T, int16_t>::value ? DHR_IDX_I16 : -1;
}

int main() {
  expect<TypeTag<char>>("pick_type 0", [](auto f) { return pick_type<char, long, double>(0, f); });
  expect<TypeTag<long>>("pick_type 1", [](auto f) { return pick_type<char, long, double>(1, f); });
  expect<TypeTag<double>>("pick_type 2", [](auto f) { return pick_type<char, long, double>(2, f); });
  for (int i : {-1, 3, 1 << 30}) expect_miss("pick_type", [i](auto f) { return pick_type<char, long, double>(i, f); });

  expect<TypeTag<float>>("value f32", [](auto f) { return with_value_type(DHR_VAL_F32, f); });
  expect<TypeTag<_Float16>>("value f16", [](auto f) { return with_value_type(DHR_VAL_F16, f); });
  for (int c : {-1, (int)DHR_VAL_BF16, 3}) expect_miss("value", [c](auto f) { return with_value_type(c, f); });

  expect<TypeTag<float>>("value_bf16 f32", [](auto f) { return with_value_type_bf16(DHR_VAL_F32, f); });
  expect<TypeTag<_Float16>>("value_bf16 f16", [](auto f) { return with_value_type_bf16(DHR_VAL_F16, f); });
  expect<TypeTag<__bf16>>("value_bf16 bf16", [](auto f) { return with_value_type_bf16(DHR_VAL_BF16, f); });
  for (int c : {-1, 3, 255}) expect_miss("value_bf16", [c](auto f) { return with_value_type_bf16(c, f); });

  expect<TypeTag<_Float16>>("half f16", [](auto f) { return with_half_type(DHR_VAL_F16, f); });
  expect<TypeTag<__bf16>>("half bf16", [](auto f) { return with_half_type(DHR_VAL_BF16, f); });
  for (int c : {-1, (int)DHR_VAL_F32, 3}) expect_miss("half", [c](auto f) { return with_half_type(c, f); });

  expect<TypeTag<uint8_t>>("index u8", [](auto f) { return with_index_type(DHR_IDX_U8, f); });
  expect<TypeTag<int8_t>>("index i8", [](auto f) { return with_index_type(DHR_IDX_I8, f); });
  expect<TypeTag<int16_t>>("index i16", [](auto f) { return with_index_type(DHR_IDX_I16, f); });
  for (int c : {-1, (int)DHR_IDX_NONE, 4}) expect_miss("index", [c](auto f) { return with_index_type(c, f); });

  expect<TypeTag<int64_t>>("id 8", [](auto f) { return with_id_type(8, f); });
  expect<TypeTag<int32_t>>("id 4", [](auto f) { return with_id_type(4, f); });
  for (int c : {0, 1, 2, 16}) expect_miss("id", [c](auto f) { return with_id_type(c, f); });

  expect<std::true_type>("flag true", [](auto f) { return with_flag(true, f); });
  expect<std::false_type>("flag false", [](auto f) { return with_flag(false, f); });

  expect<Int<2>>("int 2", [](auto f) { return with_int<2, 6, 12>(2, f); });
  expect<Int<6>>("int 6", [](auto f) { return with_int<2, 6, 12>(6, f); });
  expect<Int<12>>("int 12", [](auto f) { return with_int<2, 6, 12>(12, f); });
  expect<Int<7>>("int alone", [](auto f) { return with_int<7>(7, f); });
  for (int n : {0, 3, 7, 13, -2}) expect_miss("int", [n](auto f) { return with_int<2, 6, 12>(n, f); });

  // a lambda that returns nothing is as good
  const char* what = "void";
  int voids = 0;
  with_value_type(DHR_VAL_F16, [&](auto) { ++voids; });
  with_flag(true, [&](auto) { ++voids; });
  with_int<4, 2, 1>(1, [&](auto) { ++voids; });
  CHECK(voids == 3);

  // nested, the way the launchers use them: every combination once, each with its own types and constants, the innermost value passed out
  what = "nested";
  int seen[3][4][2][5] = {};
  long visits = 0;
  for (int v : {(int)DHR_VAL_F16, (int)DHR_VAL_F32, (int)DHR_VAL_BF16})
    for (int x : {(int)DHR_IDX_U8, (int)DHR_IDX_I8, (int)DHR_IDX_I16})
      for (int b = 0; b < 2; ++b)
        for (int r : {4, 2, 1}) {
          const int want = ((v * 4 + x) * 2 + b) * 5 + r;
          const int got = with_value_type_bf16(v, [&](auto tv) { return with_index_type(x, [&](auto ti) { return with_flag(b != 0, [&](auto fb) {
            return with_int<4, 2, 1>(r, [&](auto nr) -> int {
              using TV = typename decltype(tv)::type;
              using TI = typename decltype(ti)::type;
              constexpr int B = decltype(fb)::value, R = decltype(nr)::value;
              CHECK(val_code<TV>() == v && idx_code<TI>() == x && B == b && R == r);
              ++seen[val_code<TV>()][idx_code<TI>()][B][R];
              ++visits;
              return ((val_code<TV>() * 4 + idx_code<TI>()) * 2 + B) * 5 + R;
            });
          }); }); });
          CHECK(got == want);
          CHECK(seen[v][x][b][r] == 1);
          ++n_arms;
        }
  CHECK(visits == 3 * 3 * 2 * 3);
  // a miss in an inner dispatcher runs nothing either
  int inner = 0;
  bool threw = false;
  try {
    with_value_type(DHR_VAL_F32, [&](auto) { with_index_type(DHR_IDX_NONE, [&](auto) { ++inner; }); });
  } catch (const std::logic_error&) {
    threw = true;
  }
  CHECK(threw && inner == 0);

  std::printf("op dispatch ok: %ld arms\n", n_arms);
  return 0;
}
