// The CPU pass that option "scalars_montgomery" takes off a native caller: n scalars a = k 2^256 mod m -> canonical k, with the function of
// csrc/scalar_form.hpp compiled for the host, on T threads (contiguous slices, one per thread; in place, as a caller converting its own
// vector would).  Prints one JSON line per (modulus, T): best and median of `reps` passes.  Built and run by tools/montgomery_inputs.py:
//   g++ -O3 -march=native -std=c++17 -pthread -o montgomery_decode_bench tools/montgomery_decode_bench.cpp && ./montgomery_decode_bench 20 1 16
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <thread>
#include <vector>
#include "../webgpu-msm-twisted-edwards_amd/csrc/scalar_form.hpp"

template <int FORM> static void decode_range(uint8_t* p, size_t lo, size_t hi) {
  for (size_t i = lo; i < hi; i++) {
    uint32_t a[8];
    memcpy(a, p + 32 * i, 32);
    te::scalar_from_montgomery<FORM>(a);
    memcpy(p + 32 * i, a, 32);
  }
}

template <int FORM> static void run(const char* name, size_t n, int T, int reps) {
  std::vector<uint8_t> src(32 * n), buf(32 * n);
  uint64_t s = 0x2545f4914f6cdd1dull;
  for (size_t i = 0; i < src.size(); i += 8) { s = s * 6364136223846793005ull + 1442695040888963407ull; memcpy(&src[i], &s, 8); }
  std::vector<double> ms;
  uint32_t sink = 0;
  for (int r = 0; r < reps + 1; r++) {
    memcpy(buf.data(), src.data(), src.size());
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> th;
    for (int t = 1; t < T; t++) th.emplace_back(decode_range<FORM>, buf.data(), n * t / T, n * (t + 1) / T);
    decode_range<FORM>(buf.data(), 0, n / T);
    for (auto& x : th) x.join();
    const double d = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (r) ms.push_back(d);                                  // (the first pass warms pages and threads)
    sink ^= buf[(size_t)r * 37 % buf.size()];
  }
  std::sort(ms.begin(), ms.end());
  printf("{\"cpu_decode\": \"%s\", \"n\": %zu, \"threads\": %d, \"best_ms\": %.4f, \"median_ms\": %.4f, \"ns_per_scalar_per_thread\": %.2f, \"sink\": %u}\n",
         name, n, T, ms.front(), ms[ms.size() / 2], ms.front() * 1e6 * T / (double)n, sink);
}

int main(int argc, char** argv) {
  const int log2n = argc > 1 ? atoi(argv[1]) : 20;
  const size_t n = (size_t)1 << log2n;
  for (int i = 2; i < std::max(argc, 3); i++) {
    const int T = argc > 2 ? std::max(1, atoi(argv[i])) : 1;
    run<te::SCALAR_FORM_TE>("mod L (Twisted-Edwards BLS12)", n, T, 9);
    run<te::SCALAR_FORM_377>("mod r (BLS12-377)", n, T, 9);
  }
  return 0;
}
