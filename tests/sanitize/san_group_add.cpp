// san_group_add.cpp -- stand-alone AddressSanitizer / UndefinedBehaviorSanitizer program (its own main, no Python) for batched group
// addition and point-set sums: the lane code of csrc/group_add.hip.hpp and the sum's block (emulated as loops over its lanes), through
// the host shim tests/csrc/groupaddcheck.cpp.  Self-checks, over multiples of each curve's generator built by shared-B additions:
// (A + B) - B = A at n = 1, 7, 8, 9, 2047, 2048, 2049 and 2 x 2048 + 5, each in buffers of exactly n records; and sum(P_0 .. P_n) =
// sum(P_0 .. P_(n-1)) + P_n at n = 0, 1, 2, 255, 256, 257, on the full grid and on one block (tests/test_group_add_host.py pins both to
// the bigint models).  Built and run by tests/test_group_add_host.py:
//     g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -o san_group_add san_group_add.cpp
#include <stdio.h>
#include "../csrc/groupaddcheck.cpp"

static const uint8_t kGenTe[64] = {0xc5, 0x49, 0xbe, 0x4b, 0x84, 0x82, 0x7e, 0x13, 0xf3, 0x83, 0xdd, 0xa9, 0x33, 0x88, 0x60, 0xe7, 0x06, 0x50, 0x90, 0x0d, 0xb8, 0x94, 0xb2, 0x16, 0x07, 0x50, 0x47, 0x02, 0xeb, 0x24, 0x68, 0x03, 0xd4, 0xa9, 0xcd, 0x8b, 0x7d, 0xce, 0x0d, 0xd5, 0x55, 0xc2, 0x8b, 0xc0, 0xf4, 0x58, 0x67, 0x7f, 0xe5, 0xbc, 0x0a, 0x81, 0x1e, 0xa8, 0xc0, 0x37, 0xa3, 0x97, 0xd8, 0xc1, 0xd5, 0xd8, 0xb1, 0x11};
static const uint8_t kGen377[96] = {0xef, 0xe9, 0x1b, 0xb2, 0x6e, 0xb1, 0xb9, 0xea, 0x4e, 0x39, 0xcd, 0xff, 0x12, 0x15, 0x48, 0xd5, 0x5c, 0xcb, 0x37, 0xbd, 0xc8, 0x82, 0x82, 0x18, 0xbb, 0x41, 0x9d, 0xaa, 0x2c, 0x1e, 0x95, 0x85, 0x54, 0xff, 0x87, 0xbf, 0x25, 0x62, 0xfc, 0xc8, 0x67, 0x0a, 0x74, 0xfe, 0xde, 0x48, 0x88, 0x00, 0xa6, 0x8e, 0x9c, 0x55, 0x55, 0xde, 0x82, 0xfd, 0x1a, 0x59, 0xa9, 0x34, 0x36, 0x3d, 0xfe, 0xc2, 0x05, 0x23, 0xb8, 0x4f, 0xd4, 0x2a, 0x18, 0x6d, 0xd9, 0x52, 0x3e, 0xca, 0x48, 0xb3, 0x7f, 0xbd, 0xc4, 0xee, 0xaf, 0x30, 0x5d, 0x4f, 0x67, 0x1f, 0xff, 0x2e, 0x10, 0xc5, 0x69, 0x4a, 0x91, 0x01};

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

template <int CURVE> static void run(const uint8_t* gen) {
  using Z = ga_sizes<CURVE>;
  constexpr size_t PB = Z::PW * 4;
  const uint32_t total = 2u * 2048u + 5u;
  // pts[i] = [i + 1] G: the first k doubled in length by one shared-B addition of [k] G
  std::vector<uint8_t> pts((size_t)total * PB);
  memcpy(pts.data(), gen, PB);
  for (uint32_t k = 1; k < total; k *= 2) {
    const uint32_t cnt = std::min(k, total - k);
    add<CURVE>(pts.data(), &pts[(size_t)(k - 1) * PB], cnt, 2, 0, &pts[(size_t)k * PB]);
  }
  std::vector<uint8_t> rev((size_t)total * PB);
  for (uint32_t i = 0; i < total; i++) memcpy(&rev[(size_t)i * PB], &pts[(size_t)(total - 1u - i) * PB], PB);
  for (uint32_t m : {1u, 7u, 8u, 9u, 2047u, 2048u, 2049u, total}) {
    std::vector<uint8_t> a(pts.begin(), pts.begin() + (size_t)m * PB), bb(rev.begin(), rev.begin() + (size_t)m * PB);      // (exactly m records: a read past them is a report)
    std::vector<uint8_t> s((size_t)m * PB), back((size_t)m * PB);
    add<CURVE>(a.data(), bb.data(), m, 0, 0, s.data());
    add<CURVE>(s.data(), bb.data(), m, 1, 0, back.data());
    CHECK(back == a);
    add<CURVE>(a.data(), a.data(), m, 1, 0, back.data());                         // P - P: the identity in every record
    std::vector<uint8_t> ident(PB, 0);
    if (CURVE == 0) ident[32] = 1;
    for (uint32_t i = 0; i < m; i++) CHECK(memcmp(&back[(size_t)i * PB], ident.data(), PB) == 0);
  }
  for (uint32_t n : {0u, 1u, 2u, 255u, 256u, 257u}) {
    std::vector<uint8_t> lo(PB), hi(PB), step(PB);
    std::vector<uint8_t> exact(pts.begin(), pts.begin() + (size_t)(n + 1u) * PB);
    sum<CURVE>(exact.data(), n, 1024u, lo.data());
    sum<CURVE>(exact.data(), n + 1u, 1024u, hi.data());
    add<CURVE>(lo.data(), &exact[(size_t)n * PB], 1, 0, 0, step.data());
    CHECK(step == hi);
    sum<CURVE>(exact.data(), n + 1u, 1u, lo.data());
    CHECK(lo == hi);
  }
}

int main() {
  run<0>(kGenTe);
  run<1>(kGen377);
  if (failures) { printf("san_group_add: %d checks FAILED\n", failures); return 1; }
  printf("san_group_add: all checks passed\n");
  return 0;
}
