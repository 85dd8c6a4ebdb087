// san_field.cpp -- the batched field arithmetic (csrc/field_ops.hip.hpp) through fieldopscheck.cpp's emulation, as a program of its own
// under -fsanitize=address,undefined (tests/test_field_ops_host.py builds and runs it).  Every buffer is a heap allocation of exactly
// the bytes the call may touch, so a read or write past an element, a slab plane or a partial tile is a report; the results are checked
// by the field's own identities (a / a = 1, sqrt(a^2)^2 = a^2, a^17 by products), on both fields and in both forms.
#include "fieldopscheck.cpp"
#include <stdio.h>

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

namespace {
typedef std::vector<uint8_t> bytes;
uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint8_t next_byte() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint8_t)(rng_state >> 56); }

bytes values(int field, uint64_t n) {
  bytes v((size_t)n * (field ? 48 : 32));
  for (auto& x : v) x = next_byte();
  return v;
}
// 0 or -6; out is exactly n elements
int op(int field, int o, const bytes& a, const bytes* b, int flags, uint32_t group, bytes& out, int64_t* bad = nullptr, int* why = nullptr) {
  const uint64_t n = a.size() / (field ? 48 : 32);
  int64_t i = -1; int w = 0;
  out.assign(a.size(), 0xA5);
  const int rc = fo_field_op(field, o, a.data(), b ? b->data() : nullptr, n, flags, group, 0, out.data(), &i, &w);
  if (bad) *bad = i;
  if (why) *why = w;
  return rc;
}
}  // namespace

int main() {
  for (int field = 0; field < 2; field++)
    for (int flags = 0; flags <= F_MONT; flags += F_MONT) {
      const size_t eb = field ? 48 : 32;
      bytes one, o1, o2;
      const bytes e0(32, 0);
      CHECK(op(field, OP_POW, values(field, 1), &e0, flags | F_SHARED, 16, one) == 0, "a^0");        // 1, in the call's form
      if (!flags) { bytes plain(eb, 0); plain[0] = 1; CHECK(one == plain, "a^0 = 1"); }
      for (uint32_t group : {1u, 8u, 16u, 64u})
        for (uint64_t n : {(uint64_t)1, (uint64_t)255, (uint64_t)256 * group + 1}) {
          bytes a = values(field, n);
          memset(a.data() + (n / 2) * eb, 0, eb);                  // one zero
          int64_t bad = -1; int why = 0;
          CHECK(op(field, OP_INV, a, nullptr, flags, group, o1, &bad, &why) == -6 && bad == (int64_t)(n / 2) && why == 1, "strict inversion reports the zero");
          CHECK(o1 == bytes(a.size(), 0xA5), "output untouched");
          CHECK(op(field, OP_INV, a, nullptr, flags | F_ZERO_OK, group, o1) == 0, "inv");
          CHECK(op(field, OP_MUL, a, &o1, flags, group, o2) == 0, "mul");
          for (uint64_t i = 0; i < n; i++) {
            const bool z = i == n / 2;
            CHECK(memcmp(&o2[i * eb], z ? bytes(eb, 0).data() : one.data(), eb) == 0, "a / a = 1: field %d flags %d group %u n %llu i %llu", field, flags, group,
                  (unsigned long long)n, (unsigned long long)i);
          }
          bytes in_place = a;                                        // out == a
          int64_t i0; int w0;
          CHECK(fo_field_op(field, OP_INV, in_place.data(), nullptr, n, flags | F_ZERO_OK, group, 0, in_place.data(), &i0, &w0) == 0 && in_place == o1, "in place");
        }
      const bytes a = values(field, 9);
      bytes sq, root, again, p17, e17(32, 0), acc, tmp;
      e17[0] = 17;
      CHECK(op(field, OP_SQUARE, a, nullptr, flags, 16, sq) == 0 && op(field, OP_SQRT, sq, nullptr, flags, 16, root) == 0, "sqrt of squares");
      CHECK(op(field, OP_SQUARE, root, nullptr, flags, 16, again) == 0 && again == sq, "sqrt(a^2)^2 = a^2");
      CHECK(op(field, OP_POW, a, &e17, flags | F_SHARED, 16, p17) == 0, "pow 17");
      bytes e17n;
      for (int i = 0; i < 9; i++) e17n.insert(e17n.end(), e17.begin(), e17.end());
      CHECK(op(field, OP_POW, a, &e17n, flags, 16, tmp) == 0 && tmp == p17, "per-element exponents = the shared one");
      op(field, OP_SQUARE, a, nullptr, flags, 16, acc);              // a^2, ^4, ^8, ^16, then a
      for (int k = 0; k < 3; k++) { op(field, OP_SQUARE, acc, nullptr, flags, 16, tmp); acc = tmp; }
      CHECK(op(field, OP_MUL, acc, &a, flags, 16, tmp) == 0 && tmp == p17, "a^17 by products");
      bytes s, d, back, ng, zero;
      CHECK(op(field, OP_ADD, a, &sq, flags, 16, s) == 0 && op(field, OP_SUB, s, &sq, flags, 16, back) == 0, "add, sub");
      CHECK(op(field, OP_NEG, a, nullptr, flags, 16, ng) == 0 && op(field, OP_ADD, a, &ng, flags, 16, zero) == 0 && zero == bytes(a.size(), 0), "a + (-a) = 0");
      CHECK(op(field, OP_DOUBLE, a, nullptr, flags, 16, d) == 0 && op(field, OP_ADD, a, &a, flags, 16, tmp) == 0 && tmp == d, "2 a = a + a");
      CHECK(op(field, OP_SUB, back, &ng, flags, 16, tmp) == 0 && tmp == d, "(a + b - b) - (-a) = 2 a");
    }
  printf(fails ? "san_field: %d FAILURES\n" : "san_field ok\n", fails);
  return fails ? 1 : 0;
}
