// san_mul_base.cpp -- stand-alone AddressSanitizer / UndefinedBehaviorSanitizer program (its own main, no Python) for the fixed-base
// batch scalar multiplication: the lane code and the host-side table scalars of csrc/mul_base.hip.hpp, through the host shim
// tests/csrc/mulbasecheck.cpp.  Self-check: over the generator of each curve, [k] P from the table (mb_lane + the affine pass) equals
// [k] P from the variable-base chain (sm_point, tests/test_scalar_mul_host.py pins it to the bigint model), byte for byte, for edge
// and digit-pattern scalars at W = 4, 5 and 8, with the table built by repeated addition and, for the lowest and the top window at W = 4, by
// the chain over the table scalars, and no look-up outside the table.  Built and run by tests/test_mul_base_host.py:
//     g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -o san_mul_base san_mul_base.cpp
#include <stdio.h>
#include "../csrc/mulbasecheck.cpp"

static const uint8_t kGenTe[64] = {0xc5, 0x49, 0xbe, 0x4b, 0x84, 0x82, 0x7e, 0x13, 0xf3, 0x83, 0xdd, 0xa9, 0x33, 0x88, 0x60, 0xe7, 0x06, 0x50, 0x90, 0x0d, 0xb8, 0x94, 0xb2, 0x16, 0x07, 0x50, 0x47, 0x02, 0xeb, 0x24, 0x68, 0x03, 0xd4, 0xa9, 0xcd, 0x8b, 0x7d, 0xce, 0x0d, 0xd5, 0x55, 0xc2, 0x8b, 0xc0, 0xf4, 0x58, 0x67, 0x7f, 0xe5, 0xbc, 0x0a, 0x81, 0x1e, 0xa8, 0xc0, 0x37, 0xa3, 0x97, 0xd8, 0xc1, 0xd5, 0xd8, 0xb1, 0x11};
static const uint8_t kGen377[96] = {0xef, 0xe9, 0x1b, 0xb2, 0x6e, 0xb1, 0xb9, 0xea, 0x4e, 0x39, 0xcd, 0xff, 0x12, 0x15, 0x48, 0xd5, 0x5c, 0xcb, 0x37, 0xbd, 0xc8, 0x82, 0x82, 0x18, 0xbb, 0x41, 0x9d, 0xaa, 0x2c, 0x1e, 0x95, 0x85, 0x54, 0xff, 0x87, 0xbf, 0x25, 0x62, 0xfc, 0xc8, 0x67, 0x0a, 0x74, 0xfe, 0xde, 0x48, 0x88, 0x00, 0xa6, 0x8e, 0x9c, 0x55, 0x55, 0xde, 0x82, 0xfd, 0x1a, 0x59, 0xa9, 0x34, 0x36, 0x3d, 0xfe, 0xc2, 0x05, 0x23, 0xb8, 0x4f, 0xd4, 0x2a, 0x18, 0x6d, 0xd9, 0x52, 0x3e, 0xca, 0x48, 0xb3, 0x7f, 0xbd, 0xc4, 0xee, 0xaf, 0x30, 0x5d, 0x4f, 0x67, 0x1f, 0xff, 0x2e, 0x10, 0xc5, 0x69, 0x4a, 0x91, 0x01};

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

template <int CURVE> static void run(const uint8_t* point) {
  using Z = sm_sizes<CURVE>;
  constexpr int SB = CURVE == 1 ? 48 : 32, PB = Z::PW * 4;
  // scalars: 0, 1, 2^256 - 1, all-ones windows, alternating bytes, single high bits
  std::vector<std::vector<uint8_t>> ks;
  auto push = [&](const uint8_t (&k)[32]) { std::vector<uint8_t> r(SB, 0); memcpy(r.data(), k, 32); ks.push_back(r); };
  uint8_t k[32];
  memset(k, 0, 32); push(k);
  k[0] = 1; push(k);
  memset(k, 0xff, 32); push(k);
  memset(k, 0x77, 32); push(k);
  memset(k, 0x88, 32); push(k);
  for (int i = 0; i < 32; i++) k[i] = (i & 1) ? 0x7f : 0x80;
  push(k);
  memset(k, 0, 32); k[31] = 0x80; push(k);
  memset(k, 0, 32); k[31] = 0xf0; k[0] = 0x0f; push(k);
  for (uint32_t s = 1; s <= 4; s++) { for (int i = 0; i < 32; i++) k[i] = (uint8_t)(s * 0x9e3779b9u >> ((i * 7) % 24)) ^ (uint8_t)(i * 37u * s); push(k); }
  const uint64_t n = ks.size();
  std::vector<uint8_t> sc(n * SB), pts(n * PB), want(n * PB), got(n * PB);
  for (uint64_t i = 0; i < n; i++) { memcpy(&sc[i * SB], ks[i].data(), SB); memcpy(&pts[i * PB], point, PB); }
  {
    std::vector<uint32_t> proj((size_t)n * Z::JW);
    const naf_t kn = {};
    for (uint64_t i = 0; i < n; i++) {
      uint32_t w[Z::PW], kw[8];
      memcpy(w, point, PB); memcpy(kw, &sc[i * SB], 32);
      sm_point<CURVE, false>(w, kw, kn, &proj[i * Z::JW]);
    }
    affine_pass<CURVE>(proj, n, want.data());
  }
  for (int W : {4, 5, 8}) {
    const mb_geom g = mb_geometry(W);
    std::vector<uint8_t> tab((size_t)g.entries * MB_SLOT_WORDS * 4);
    mbc_table_by_addition(CURVE, W, point, tab.data());
    if (W == 4) {
      std::vector<uint8_t> s32((size_t)g.entries * 32);                        // (the chain is slow under the sanitizers: windows 0 and M - 1)
      mbc_table_scalars(CURVE, W, s32.data());
      for (uint32_t first : {0u, g.entries - (g.H + 1u)}) {
        std::vector<uint8_t> part((size_t)(g.H + 1u) * MB_SLOT_WORDS * 4);
        mbc_table_from_scalars(CURVE, point, &s32[(size_t)first * 32], g.H + 1u, part.data());
        CHECK(memcmp(part.data(), &tab[(size_t)first * MB_SLOT_WORDS * 4], part.size()) == 0);
      }
    }
    std::vector<int32_t> digits(g.M);
    mbc_digits(W, ks[2].data(), digits.data());
    CHECK(digits[g.M - 1] >= 0);
    mbc_mul(CURVE, 0, W, tab.data(), nullptr, sc.data(), n, got.data());
    CHECK(got == want);
  }
  CHECK(mbc_out_of_table() == 0);
}

int main() {
  run<0>(kGenTe);
  run<1>(kGen377);
  if (failures) { printf("san_mul_base: %d checks FAILED\n", failures); return 1; }
  printf("san_mul_base: all checks passed\n");
  return 0;
}
