// san_ntt.cpp -- the NTT (csrc/ntt.hip.hpp, csrc/ntt_plan.hpp) through nttcheck.cpp's emulation, as a program of its own under
// -fsanitize=address,undefined (tests/test_ntt_host.py builds and runs it).  Every buffer is a heap allocation of exactly the bytes the
// call may touch, so a read or write past a record, a table entry, an LDS slot or a partly filled tile is a report; the results are
// held against the shim's textbook transform and against the transform's own identities (the inverse undoes the forward, all ones
// -> n delta_0), in both forms, with and without a shift, at one, two and three passes and across the piece loop.
#include "nttcheck.cpp"
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
int emu(const bytes& a, uint32_t log_n, uint64_t count, int flags, const uint8_t* shift, uint64_t piece, bytes& out) {
  out.assign(a.size(), 0xA5);
  return ntt_emulate(a.data(), log_n, count, flags, shift, 0, piece, out.data(), nullptr);
}
}  // namespace

int main() {
  uint8_t s22[32] = {22}, s_big[32];
  memset(s_big, 0xff, 32);
  const struct { uint32_t log_n; uint64_t count, piece; } cases[] = {{0, 1025, 0}, {3, 129, 0}, {5, 3, 2}, {10, 2, 0}, {11, 3, 2}, {17, 1, 0}};
  int turn = 0;
  for (const auto& c : cases)
    for (int flags = 0; flags < 4; flags++, turn++) {
      const uint8_t* const shifts[3] = {nullptr, s22, s_big};
      {
        const uint8_t* shift = shifts[turn % 3];                     // (every direction and form at every size; the shifts come round)
        if (c.log_n >= 16 && flags != 0 && flags != 3) continue;     // three passes: forward plain, inverse Montgomery
        const bytes a = values(c.count << c.log_n);
        bytes want(a.size()), got, back;
        CHECK(ntt_ref(a.data(), c.log_n, c.count, flags, shift, want.data()) == 0, "ref");
        CHECK(emu(a, c.log_n, c.count, flags, shift, c.piece, got) == 0 && got == want, "emulation = textbook: log_n %u count %llu flags %d", c.log_n,
              (unsigned long long)c.count, flags);
        if (c.log_n >= 16) continue;                                 // (three passes: the comparison above is the check)
        bytes in_place = a;
        CHECK(ntt_emulate(in_place.data(), c.log_n, c.count, flags, shift, 0, c.piece, in_place.data(), nullptr) == 0 && in_place == want, "in place: log_n %u", c.log_n);
        CHECK(emu(got, c.log_n, c.count, flags ^ 1, shift, c.piece, back) == 0, "the other direction");
        bytes canon(a.size()), again;                                  // a itself, reduced: the copy at log_n = 0 in the same form
        CHECK(ntt_ref(a.data(), 0, c.count << c.log_n, flags & 2, nullptr, canon.data()) == 0 && back == canon, "inverse(forward(a)) = a: log_n %u flags %d", c.log_n, flags);
      }
    }
  for (uint32_t log_n : {0u, 4u, 10u, 11u, 17u}) {
    bytes ones((size_t)32 << log_n, 0), out, want((size_t)32 << log_n, 0);
    for (uint64_t i = 0; i < (1ull << log_n); i++) ones[32 * i] = 1;
    const uint64_t n = 1ull << log_n;
    memcpy(want.data(), &n, 8);
    CHECK(emu(ones, log_n, 1, 0, nullptr, 0, out) == 0 && out == want, "all ones -> n delta_0: log_n %u", log_n);
  }
  bytes a = values(8), out;
  uint8_t zero[32] = {};
  int why = 0;
  out.assign(a.size(), 0xA5);
  CHECK(ntt_emulate(a.data(), 3, 1, 0, zero, 0, 0, out.data(), &why) == -1 && why == NTT_ZERO_SHIFT && out == bytes(a.size(), 0xA5), "a zero shift is refused, the output untouched");
  CHECK(ntt_emulate(a.data(), 25, 1, 0, nullptr, 0, 0, out.data(), &why) == -1 && why == NTT_BAD_LOG_N && out == bytes(a.size(), 0xA5), "log_n 25 is refused");
  uint64_t checked = 0;
  for (uint32_t log_n : {0u, 7u, 10u, 11u, 16u, 17u}) CHECK(ntt_replay(log_n, log_n < 10 ? 1500 : 2, &checked) == 0, "replay %u", log_n);
  printf(fails ? "san_ntt: %d FAILURES\n" : "san_ntt ok\n", fails);
  return fails ? 1 : 0;
}
