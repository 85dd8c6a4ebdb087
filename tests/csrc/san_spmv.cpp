// san_spmv.cpp -- the sparse matrix-vector product (csrc/spmv.hip.hpp, csrc/spmv_plan.hpp) through spmvcheck.cpp's emulation, as a program
// of its own under -fsanitize=address,undefined (tests/test_spmv_host.py builds and runs it).  Every buffer is a heap allocation of exactly
// the bytes the call may touch, so a read or write past a record, a row id, a fragment or an LDS word is a report; the results are held
// against the definition itself, summed here entry by entry with the host build of the field, for the matrix and its transpose, at
// chunk 1, 4 and the default, over short rows, empty rows, rows that span tiles and one row that holds everything.
#include "spmvcheck.cpp"
#include <stdio.h>

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

namespace {
typedef std::vector<uint8_t> bytes;
uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t next_u32() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 32); }
bytes values(uint64_t n) {
  bytes v((size_t)n * 32);
  for (auto& x : v) x = (uint8_t)(next_u32() >> 24);
  return v;
}
struct csr { uint64_t rows, cols; std::vector<uint64_t> ptr; std::vector<uint32_t> col; bytes vals; };
// rows of the given lengths, columns by a stride that repeats and descends
csr matrix_of(const std::vector<uint64_t>& lens, uint64_t cols) {
  csr m; m.rows = lens.size(); m.cols = cols; m.ptr.push_back(0);
  for (uint64_t n : lens) m.ptr.push_back(m.ptr.back() + n);
  const uint64_t nnz = m.ptr.back();
  m.col.resize(nnz);
  for (uint64_t e = 0; e < nnz; e++) m.col[e] = (uint32_t)((nnz - e) * 7u % cols);
  m.vals = values(nnz);
  return m;
}
// the definition, entry by entry: out[r] (or out[c] under `tr`) += v x, everything canonical at the end
bytes direct(const csr& m, const bytes& x, uint64_t count, bool tr) {
  const uint64_t n_in = tr ? m.rows : m.cols, n_out = tr ? m.cols : m.rows;
  std::vector<fel<9>> acc((size_t)(count * n_out), fe_zero<9>());
  for (uint64_t k = 0; k < count; k++)
    for (uint64_t r = 0; r < m.rows; r++)
      for (uint64_t e = m.ptr[r]; e < m.ptr[r + 1]; e++) {
        uint32_t vw[8], xw[8];
        memcpy(vw, m.vals.data() + e * 32, 32);
        memcpy(xw, x.data() + (k * n_in + (tr ? r : m.col[e])) * 32, 32);
        fel<9>& a = acc[(size_t)(k * n_out + (tr ? m.col[e] : r))];
        a = fo_residue(fe_norm(fe_add(a, fe_mul(fo_decode<9, false>(vw), fp_from_words32(xw)))));
      }
  bytes out((size_t)(count * n_out) * 32);
  for (size_t i = 0; i < acc.size(); i++) { uint32_t w[8]; fo_words<9, 8>(fo_residue(acc[i]), w); memcpy(out.data() + i * 32, w, 32); }
  return out;
}
}  // namespace

int main() {
  for (uint32_t chunk : {1u, 4u, 0u}) {
    const uint64_t T = 256u * (chunk ? chunk : te_spmv::kChunkDefault);
    const std::vector<std::vector<uint64_t>> shapes = {
        {1}, {0, 0, 3, 0, 5, 0}, std::vector<uint64_t>(T + 9, 1), {2 * T + 300}, {T + T / 2, 3, 1, 0, 5, 2, T, 4}, {3, 3 * T + 10, 2}, {T - 3, 3, 0, 0, 0, 7, 0, T - 7, 0, 0, 4}, {0, 0}};
    for (const auto& lens : shapes) {
      const csr m = matrix_of(lens, 61);
      for (int tr = 0; tr < 2; tr++)
        for (uint64_t count : {1ull, 3ull}) {
          const uint64_t n_in = tr ? m.rows : m.cols, n_out = tr ? m.cols : m.rows;
          const bytes x = values(count * n_in);
          bytes out((size_t)(count * n_out) * 32, 0xA5);
          int why = 0; int64_t bad = -1;
          const int rc = spmv_emulate(m.rows, m.cols, m.ptr.data(), m.col.data(), m.vals.data(), tr ? TE_MSM_MATRIX_TRANSPOSE : 0, x.data(), count, tr ? TE_MSM_SPMV_TRANSPOSE : 0, chunk, 0,
                                      out.data(), &why, &bad);
          CHECK(rc == 0, "emulate rc %d: rows %llu nnz %llu chunk %u tr %d", rc, (unsigned long long)m.rows, (unsigned long long)m.ptr.back(), chunk, tr);
          CHECK(out == direct(m, x, count, tr != 0), "the definition: rows %llu nnz %llu chunk %u tr %d count %llu", (unsigned long long)m.rows, (unsigned long long)m.ptr.back(), chunk, tr,
                (unsigned long long)count);
        }
    }
  }
  {
    const csr m = matrix_of({3, 0, 4}, 5);
    const bytes x = values(5);
    bytes out(3 * 32, 0xA5);
    const bytes keep = out;
    int why = 0; int64_t bad = -1;
    std::vector<uint32_t> col = m.col;
    col[4] = 5; col[6] = 9;
    CHECK(spmv_emulate(3, 5, m.ptr.data(), col.data(), m.vals.data(), 0, x.data(), 1, 0, 0, 0, out.data(), &why, &bad) == -1 && why == SPMV_BAD_INDEX && bad == 4 && out == keep,
          "a column index out of range is refused at its lowest position");
    CHECK(spmv_emulate(3, 5, m.ptr.data(), m.col.data(), m.vals.data(), 0, x.data(), 1, TE_MSM_SPMV_TRANSPOSE, 0, 0, out.data(), &why, &bad) == -1 && why == SPMV_NO_TRANSPOSE && out == keep,
          "TRANSPOSE without the bind's flag is refused");
    CHECK(spmv_emulate(3, 5, m.ptr.data(), m.col.data(), m.vals.data(), 8, x.data(), 1, 0, 0, 0, out.data(), &why, &bad) == -1 && why == SPMV_BAD_FLAGS && out == keep, "an unknown flag is refused");
  }
  uint64_t checked = 0;
  for (uint64_t nnz : {0ull, 1ull, 256ull, 257ull, 65537ull, (1ull << 24) + 1ull}) CHECK(spmv_replay(1000, 77, nnz, 3, 1, &checked) == 0, "replay %llu", (unsigned long long)nnz);
  printf(fails ? "san_spmv: %d FAILURES\n" : "san_spmv ok\n", fails);
  return fails ? 1 : 0;
}
