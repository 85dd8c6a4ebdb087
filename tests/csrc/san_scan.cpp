// san_scan.cpp -- prefix sums and products (csrc/scan.hip.hpp, csrc/scan_plan.hpp) through scancheck.cpp's emulation, as a program of its
// own under -fsanitize=address,undefined (tests/test_scan_host.py builds and runs it).  Every buffer is a heap allocation of exactly the
// bytes the call may touch, so a read or write past a record, a seed, an LDS word or a partly filled tile is a report; the results are
// held against the definition itself, walked here with the host build of the field: next = previous o a_i from the seed, every output
// canonical, in both ops, modes and forms, at one, two and three levels, shared and not, in place and out of place.
#include "scancheck.cpp"
#include <stdio.h>

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

namespace {
typedef std::vector<uint8_t> bytes;
uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint8_t next_byte() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint8_t)(rng_state >> 56); }
bytes values(uint64_t n) {
  bytes v((size_t)n * 32);
  for (auto& x : v) x = next_byte();
  return v;
}
// the canonical words of prev o a in the caller's form (mont: x A * y A / A)
void step(int op, bool mont, const uint8_t* prev, const uint8_t* a, uint32_t (&o)[8]) {
  uint32_t wp[8], wa[8];
  memcpy(wp, prev, 32); memcpy(wa, a, 32);
  if (op == TE_MSM_SCAN_SUM) fo_map<9, FO_ADD, false>(wp, wa, o);
  else if (mont) fo_map<9, FO_MUL, true>(wp, wa, o);
  else fo_map<9, FO_MUL, false>(wp, wa, o);
}
bool definition_holds(int op, const bytes& a, uint64_t n, uint64_t count, int flags, const bytes* init, const bytes& out, const bytes& tot) {
  const bool mont = flags & TE_MSM_SCAN_MONTGOMERY, excl = flags & TE_MSM_SCAN_EXCLUSIVE, shared = flags & TE_MSM_SCAN_SHARED_A;
  for (uint64_t k = 0; k < count; k++) {
    uint8_t cur[32] = {};
    uint32_t o[8];
    if (init) memcpy(cur, init->data() + k * 32, 32);
    else if (op == TE_MSM_SCAN_PRODUCT) { fel<9> one = fe_one<9>(); if (mont) fo_encode<9, true>(one, o); else fo_encode<9, false>(one, o); memcpy(cur, o, 32); }
    { const uint8_t zero[32] = {}; step(TE_MSM_SCAN_SUM, false, cur, zero, o); memcpy(cur, o, 32); }      // the seed, canonical
    for (uint64_t i = 0; i < n; i++) {
      const uint8_t* rec = out.data() + (k * n + i) * 32;
      if (excl && memcmp(rec, cur, 32)) return false;
      step(op, mont, cur, a.data() + (shared ? k : k * n + i) * 32, o);
      memcpy(cur, o, 32);
      if (!excl && memcmp(rec, cur, 32)) return false;
    }
    if (memcmp(tot.data() + k * 32, cur, 32)) return false;
  }
  return true;
}
}  // namespace

int main() {
  const struct { uint64_t n, count; uint32_t chunk; } cases[] = {{1, 5, 1}, {255, 2, 1}, {257, 3, 1}, {65537, 1, 1}, {1023, 2, 4}, {2 * 1024 + 300, 3, 4},
                                                                 {2049, 2, 0}, {16 * 256 + 1, 1, 16}};
  for (const auto& c : cases)
    for (int op = 0; op < 2; op++)
      for (int flags = 0; flags < 8; flags++) {
        if (c.n > 60000 && flags != 0 && flags != 7) continue;
        const bool shared = flags & TE_MSM_SCAN_SHARED_A;
        const bytes a = values(shared ? c.count : c.n * c.count), init = values(c.count);
        const bytes* seed = (flags + op) & 1 ? &init : nullptr;
        const size_t ob = (size_t)c.n * c.count * 32;
        bytes tot(c.count * 32, 0xA5), out(ob, 0xA5), tot2(c.count * 32, 0xA5), tot3(c.count * 32, 0xA5), out2(ob, 0xA5);
        CHECK(scan_emulate(op, a.data(), c.n, c.count, flags, c.chunk, 0, seed ? seed->data() : nullptr, tot.data(), out.data(), nullptr) == 0, "emulate n %llu", (unsigned long long)c.n);
        CHECK(definition_holds(op, a, c.n, c.count, flags, seed, out, tot), "the definition: op %d n %llu count %llu flags %d chunk %u", op, (unsigned long long)c.n,
              (unsigned long long)c.count, flags, c.chunk);
        if (!shared) {
          bytes in_place = a;
          CHECK(scan_emulate(op, in_place.data(), c.n, c.count, flags, c.chunk, 0, seed ? seed->data() : nullptr, tot2.data(), in_place.data(), nullptr) == 0 && in_place == out && tot2 == tot,
                "in place: n %llu", (unsigned long long)c.n);
        }
        CHECK(scan_emulate(op, a.data(), c.n, c.count, flags, c.chunk, 0, seed ? seed->data() : nullptr, tot3.data(), nullptr, nullptr) == 0 && tot3 == tot, "totals only: n %llu",
              (unsigned long long)c.n);
        CHECK(scan_emulate(op, a.data(), c.n, c.count, flags, c.chunk, 0, seed ? seed->data() : nullptr, nullptr, out2.data(), nullptr) == 0 && out2 == out, "out only: n %llu",
              (unsigned long long)c.n);
      }
  {
    const bytes a = values(8);
    bytes tot(32, 0xA5), out(a.size(), 0xA5);
    int why = 0;
    CHECK(scan_emulate(0, a.data(), 0, 1, 0, 0, 0, nullptr, tot.data(), out.data(), &why) == -1 && why == SCAN_BAD_N && out == bytes(a.size(), 0xA5) && tot == bytes(32, 0xA5), "n = 0 is refused");
    CHECK(scan_emulate(0, a.data(), 8, 1, 8, 0, 0, nullptr, tot.data(), out.data(), &why) == -1 && why == SCAN_BAD_FLAGS && out == bytes(a.size(), 0xA5), "an unknown flag is refused");
    CHECK(scan_emulate(2, a.data(), 8, 1, 0, 0, 0, nullptr, tot.data(), out.data(), &why) == -1 && why == SCAN_BAD_OP && out == bytes(a.size(), 0xA5), "an unknown op is refused");
    CHECK(scan_emulate(1, a.data(), 8, 1, 0, 0, 0, nullptr, nullptr, nullptr, &why) == -1 && why == SCAN_NO_OUTPUT, "no output is refused");
  }
  uint64_t checked = 0;
  for (uint64_t n : {1ull, 256ull, 257ull, 65537ull, (1ull << 24) + 1ull}) CHECK(scan_replay(n, 3, 1, n & 1, &checked) == 0, "replay %llu", (unsigned long long)n);
  printf(fails ? "san_scan: %d FAILURES\n" : "san_scan ok\n", fails);
  return fails ? 1 : 0;
}
