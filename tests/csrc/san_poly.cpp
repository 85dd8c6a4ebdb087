// san_poly.cpp -- the polynomial opening (csrc/poly.hip.hpp, csrc/poly_plan.hpp) through polycheck.cpp's emulation, as a program of its
// own under -fsanitize=address,undefined (tests/test_poly_host.py builds and runs it).  Every buffer is a heap allocation of exactly the
// bytes the call may touch, so a read or write past a record, a power entry, an LDS word or a partly filled tile is a report; the results
// are held against the recurrence itself, walked here with the host build of the field: q_(i-1) - z q_i = a_i with q_(-1) = a(z) and
// q_(n-1) = 0, in both forms, at one, two and three levels, with one point each and a shared one, in place and out of place.
#include "polycheck.cpp"
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
// canonical words of x - z y - a (all in one form: the check is linear) are 0
bool closes(const uint8_t* x, const fel<9>& zr, const uint8_t* y, const uint8_t* a) {
  uint32_t wx[8], wy[8], wa[8], o[8];
  memcpy(wx, x, 32); memcpy(wy, y, 32); memcpy(wa, a, 32);
  const fel<9> rhs = fo_residue(fe_norm(fe_add(fp_from_words32(wa), fe_mul(zr, fp_from_words32(wy)))));
  fo_words<9, 8>(fo_residue(fe_norm(fe_sub<2>(fp_from_words32(wx), rhs))), o);
  for (int k = 0; k < 8; k++) if (o[k]) return false;
  return true;
}
bool recurrence_holds(const bytes& a, uint64_t n, uint64_t count, const bytes& z, int flags, const bytes& ev, const bytes& q) {
  const uint8_t zero[32] = {};
  for (uint64_t k = 0; k < count; k++) {
    uint32_t w[8];
    memcpy(w, z.data() + ((flags & TE_MSM_POLY_SHARED_Z) ? 0 : 32 * k), 32);
    const fel<9> zr = (flags & TE_MSM_POLY_MONTGOMERY) ? fo_decode<9, true>(w) : fo_decode<9, false>(w);
    if (memcmp(q.data() + (k * n + n - 1) * 32, zero, 32)) return false;
    for (uint64_t i = 0; i < n; i++) {
      const uint8_t* prev = i ? q.data() + (k * n + i - 1) * 32 : ev.data() + k * 32;
      if (!closes(prev, zr, q.data() + (k * n + i) * 32, a.data() + (k * n + i) * 32)) return false;
    }
  }
  return true;
}
}  // namespace

int main() {
  const struct { uint64_t n, count; uint32_t chunk; } cases[] = {{1, 5, 1}, {255, 2, 1}, {257, 3, 1}, {65537, 1, 1}, {1023, 2, 4}, {2 * 1024 + 300, 3, 4},
                                                                 {2049, 2, 0}, {16 * 256 + 1, 1, 16}};
  for (const auto& c : cases)
    for (int flags = 0; flags < 4; flags++) {
      if (c.n > 60000 && flags != 0 && flags != 3) continue;
      const bytes a = values(c.n * c.count), z = values((flags & TE_MSM_POLY_SHARED_Z) ? 1 : c.count);
      bytes ev(c.count * 32, 0xA5), q(a.size(), 0xA5), ev2(c.count * 32, 0xA5), in_place = a, ev3(c.count * 32, 0xA5);
      CHECK(poly_emulate(a.data(), c.n, c.count, z.data(), flags, c.chunk, 0, ev.data(), q.data(), nullptr) == 0, "emulate n %llu", (unsigned long long)c.n);
      CHECK(recurrence_holds(a, c.n, c.count, z, flags, ev, q), "the recurrence: n %llu count %llu flags %d chunk %u", (unsigned long long)c.n, (unsigned long long)c.count, flags, c.chunk);
      CHECK(poly_emulate(in_place.data(), c.n, c.count, z.data(), flags, c.chunk, 0, ev2.data(), in_place.data(), nullptr) == 0 && in_place == q && ev2 == ev, "in place: n %llu",
            (unsigned long long)c.n);
      CHECK(poly_emulate(a.data(), c.n, c.count, z.data(), flags, c.chunk, 0, ev3.data(), nullptr, nullptr) == 0 && ev3 == ev, "evaluation only: n %llu", (unsigned long long)c.n);
      bytes q2(a.size(), 0xA5);
      CHECK(poly_emulate(a.data(), c.n, c.count, z.data(), flags, c.chunk, 0, nullptr, q2.data(), nullptr) == 0 && q2 == q, "quotient only: n %llu", (unsigned long long)c.n);
    }
  {
    const bytes a = values(8), z = values(1);
    bytes ev(32, 0xA5), q(a.size(), 0xA5);
    int why = 0;
    CHECK(poly_emulate(a.data(), 0, 1, z.data(), 0, 0, 0, ev.data(), q.data(), &why) == -1 && why == POLY_BAD_N && q == bytes(a.size(), 0xA5) && ev == bytes(32, 0xA5), "n = 0 is refused");
    CHECK(poly_emulate(a.data(), 8, 1, z.data(), 8, 0, 0, ev.data(), q.data(), &why) == -1 && why == POLY_BAD_FLAGS && q == bytes(a.size(), 0xA5), "an unknown flag is refused");
    CHECK(poly_emulate(a.data(), 8, 1, z.data(), 0, 0, 0, nullptr, nullptr, &why) == -1 && why == POLY_NO_OUTPUT, "no output is refused");
  }
  uint64_t checked = 0;
  for (uint64_t n : {1ull, 256ull, 257ull, 65537ull, (1ull << 24) + 1ull}) CHECK(poly_replay(n, 3, 1, 0, &checked) == 0, "replay %llu", (unsigned long long)n);
  printf(fails ? "san_poly: %d FAILURES\n" : "san_poly ok\n", fails);
  return fails ? 1 : 0;
}
