// csrc/pxr_scan.h as host code over the stand-in runtime (on_host.h, hip/hip_runtime.h): the header has no entry point of its own,
// so this file wraps its two block functions in a kernel (each called twice in a row on the same s_part: the reuse barrier) and
// exports that kernel and k_exclusive_scan by workgroup size and element types for tests/test_scan_lanes_cpu.py.
// With -DSCAN_ON_HOST_MAIN: a stand-alone program (for -fsanitize=address,undefined builds) that runs the same sizes with every
// array allocated at its exact size -- n elements where no total is asked for -- against a serial loop, and prints the counts.
#include "on_host.h"
#include "pxr_scan.h"

namespace {

// in[2][THREADS] -> out[6][THREADS]: prefix and total of in[0], prefix and total of in[1], sum of in[0], sum of in[1]
template <int THREADS, class T>
__global__ void k_block_functions(const T* in, T* out) {
  __shared__ T s_part[THREADS / 64];
  const int t = threadIdx.x;
  T total;
  out[t] = pxr::block_exclusive_scan<THREADS>(in[t], s_part, total);
  out[THREADS + t] = total;
  out[2 * THREADS + t] = pxr::block_exclusive_scan<THREADS>(in[THREADS + t], s_part, total);
  out[3 * THREADS + t] = total;
  out[4 * THREADS + t] = pxr::block_int_sum<THREADS>(in[t], s_part);
  out[5 * THREADS + t] = pxr::block_int_sum<THREADS>(in[THREADS + t], s_part);
}

template <int THREADS, class T>
void block_functions(const void* in, void* out) {
  hipLaunchKernelGGL((k_block_functions<THREADS, T>), dim3(1), dim3(THREADS), 0, nullptr, (const T*)in, (T*)out);
}
template <int THREADS, class IN, class OUT>
void scan(int64_t n, const void* in, void* out, int write_total) {
  hipLaunchKernelGGL((pxr::k_exclusive_scan<THREADS, IN, OUT>), dim3(1), dim3(THREADS), 0, nullptr, n, (const IN*)in, (OUT*)out, write_total);
}
// f(constant THREADS) for threads in {64, 256, 1024}
template <class F>
int for_threads(int threads, F f) {
  if (threads == 64) f(std::integral_constant<int, 64>());
  else if (threads == 256) f(std::integral_constant<int, 256>());
  else if (threads == 1024) f(std::integral_constant<int, 1024>());
  else return pxr::set_error(-1, "threads = %d is not 64, 256 or 1024", threads);
  return 0;
}

}  // namespace

// type: 0 int, 1 uint32_t, 2 long long
extern "C" int emu_scan_block(int threads, int type, const void* in, void* out) {
  if (type < 0 || type > 2) return pxr::set_error(-1, "type = %d", type);
  return for_threads(threads, [&](auto th) {
    constexpr int TH = decltype(th)::value;
    if (type == 0) block_functions<TH, int>(in, out);
    else if (type == 1) block_functions<TH, uint32_t>(in, out);
    else block_functions<TH, long long>(in, out);
  });
}

// types: 0 int32_t -> int64_t, 1 int -> int, 2 uint32_t -> uint32_t (the last two may run in place: in == out)
extern "C" int emu_scan_kernel(int threads, int types, int64_t n, const void* in, void* out, int write_total) {
  if (types < 0 || types > 2 || n < 0) return pxr::set_error(-1, "types = %d, n = %lld", types, (long long)n);
  return for_threads(threads, [&](auto th) {
    constexpr int TH = decltype(th)::value;
    if (types == 0) scan<TH, int32_t, int64_t>(n, in, out, write_total);
    else if (types == 1) scan<TH, int, int>(n, in, out, write_total);
    else scan<TH, uint32_t, uint32_t>(n, in, out, write_total);
  });
}

#ifdef SCAN_ON_HOST_MAIN
namespace {
uint32_t g_state = 77u;
uint32_t next() { g_state = g_state * 1664525u + 1013904223u; return g_state >> 4; }

// values of type T: small and of both signs for the signed types (no signed overflow), the full range for uint32_t (sums wrap)
template <class T> T value() { return std::is_signed<T>::value ? (T)(next() % 2001u) - (T)1000 : (T)(next() * 977u); }

template <int THREADS, class T>
int block_case() {
  std::vector<T> in(2 * THREADS), out(6 * THREADS);
  for (T& v : in) v = value<T>();
  block_functions<THREADS, T>(in.data(), out.data());
  int wrong = 0;
  for (int half = 0; half < 2; ++half) {
    T run = 0;
    for (int t = 0; t < THREADS; ++t) { wrong += out[(2 * half) * THREADS + t] != run; run += in[half * THREADS + t]; }
    for (int t = 0; t < THREADS; ++t) wrong += (out[(2 * half + 1) * THREADS + t] != run) + (out[(4 + half) * THREADS + t] != run);
  }
  return wrong;
}

template <int THREADS, class IN, class OUT>
int scan_case(int64_t n, bool in_place, int write_total) {
  std::vector<IN> in((size_t)n);
  for (IN& v : in) v = sizeof(OUT) > sizeof(IN) ? (IN)(next() >> 1 | 1u << 30) : value<IN>();   // widening: counts whose sum passes 2^32
  std::vector<OUT> expect((size_t)n + 1), out((size_t)n + (write_total ? 1 : 0));
  OUT run = 0;
  for (int64_t i = 0; i < n; ++i) { expect[(size_t)i] = run; run += (OUT)in[(size_t)i]; }
  expect[(size_t)n] = run;
  if (in_place && n > 0) memcpy(out.data(), in.data(), sizeof(IN) * (size_t)n);
  scan<THREADS, IN, OUT>(n, in_place ? (const void*)out.data() : (const void*)in.data(), out.data(), write_total);
  int wrong = 0;
  for (size_t i = 0; i < out.size(); ++i) wrong += out[i] != expect[i];
  return wrong;
}

template <int THREADS>
void all_cases(int& cases, int& wrong) {
  wrong += block_case<THREADS, int>() + block_case<THREADS, uint32_t>() + block_case<THREADS, long long>();
  cases += 3;
  for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)THREADS - 1, (int64_t)THREADS, (int64_t)THREADS + 1, (int64_t)3 * THREADS + 5, (int64_t)40 * THREADS + 3})
    for (int write_total = 0; write_total < 2; ++write_total) {
      wrong += scan_case<THREADS, int32_t, int64_t>(n, false, write_total);
      wrong += scan_case<THREADS, int, int>(n, true, write_total);
      wrong += scan_case<THREADS, uint32_t, uint32_t>(n, true, write_total);
      cases += 3;
    }
}
}  // namespace

int main() {
  int cases = 0, wrong = 0;
  all_cases<64>(cases, wrong);
  all_cases<256>(cases, wrong);
  all_cases<1024>(cases, wrong);
  printf("cases %d wrong %d\n", cases, wrong);
  return 0;
}
#endif
