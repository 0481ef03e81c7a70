// Stand-alone check of csrc/qap_csc.h (the host side of the R1CS -> QAP build): the validation and the CSR -> column-wise transposition against a naive
// transpose.  tests/test_qap_csc_host.py compiles this with -fsanitize=address,undefined and runs it; exit status 0 = every check held.
#include <cstdio>
#include <cstdint>
#include <vector>
#include <tuple>
#include <algorithm>
#include "qap_csc.h"

using namespace zkt;

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } } while (0)

static const size_t MAX_N = 8192, MAX_CELLS = (size_t)1 << 26;

struct Csr {
  size_t n, cols;
  std::vector<uint64_t> rowptr; std::vector<uint32_t> col; std::vector<uint64_t> val;
};
typedef std::tuple<uint32_t, uint32_t, uint64_t> Entry;      // row, col, value tag

// rows of (col, tag) lists -> CSR; entry k's value is {tag, k, ~tag, 7}
static Csr make(size_t n, size_t cols, const std::vector<std::vector<std::pair<uint32_t, uint64_t>>>& rows) {
  Csr m; m.n = n; m.cols = cols; m.rowptr.push_back(0);
  for (size_t j = 0; j < n; ++j) {
    if (j < rows.size()) for (auto& e : rows[j]) { m.col.push_back(e.first); const uint64_t k = m.col.size() - 1; m.val.insert(m.val.end(), {e.second, k, ~e.second, 7}); }
    m.rowptr.push_back(m.col.size());
  }
  return m;
}

// the transposition checked against a naive one: for every column, the entries of the CSR with that column, in row order then input order
static void check_transpose(const Csr& m) {
  size_t bad = 123;
  const uint32_t* col = m.col.empty() ? nullptr : m.col.data(); const uint64_t* val = m.val.empty() ? nullptr : m.val.data();
  CHECK(qap_csr_valid(m.rowptr.data(), col, val, m.n, m.cols, &bad));
  CHECK(bad == QAP_NO_ROW);
  QapCsc t;
  qap_csr_to_csc(m.rowptr.data(), col, val, m.n, m.cols, t);
  const size_t nnz = m.col.size();
  CHECK(t.colptr.size() == m.cols + 1 && t.row.size() == nnz && t.val.size() == nnz * 4);
  CHECK(t.colptr[0] == 0 && t.colptr[m.cols] == nnz);
  size_t d = 0;
  for (size_t i = 0; i < m.cols; ++i) {
    CHECK(t.colptr[i] == d);
    for (size_t j = 0; j < m.n; ++j)
      for (uint64_t k = m.rowptr[j]; k < m.rowptr[j + 1]; ++k)
        if (m.col[k] == i) {
          CHECK(d < nnz && t.row[d] == j);
          for (int w = 0; w < 4; ++w) CHECK(d < nnz && t.val[d * 4 + w] == m.val[k * 4 + w]);
          ++d;
        }
  }
  CHECK(d == nnz);
}

static void expect_invalid(const Csr& m, const uint64_t* rowptr, const uint32_t* col, const uint64_t* val, size_t want_row) {
  size_t bad = 123;
  CHECK(!qap_csr_valid(rowptr, col, val, m.n, m.cols, &bad));
  CHECK(bad == want_row);
}

int main() {
  // ---- dimensions ----
  CHECK(qap_dims_valid(1, 1, MAX_N, MAX_CELLS) && qap_dims_valid(MAX_N, MAX_CELLS / MAX_N, MAX_N, MAX_CELLS) && qap_dims_valid(1, MAX_CELLS, MAX_N, MAX_CELLS));
  CHECK(!qap_dims_valid(0, 5, MAX_N, MAX_CELLS) && !qap_dims_valid(5, 0, MAX_N, MAX_CELLS));
  CHECK(!qap_dims_valid(MAX_N + 1, 1, MAX_N, MAX_CELLS));
  CHECK(!qap_dims_valid(265, 253241, MAX_N, MAX_CELLS) && (size_t)265 * 253241 == MAX_CELLS + 1);      // cols * n = 2^26 + 1
  CHECK(!qap_dims_valid(MAX_N, MAX_CELLS / MAX_N + 1, MAX_N, MAX_CELLS) && !qap_dims_valid(1, MAX_CELLS + 1, MAX_N, MAX_CELLS));
  CHECK(!qap_dims_valid(3, ~(size_t)0, MAX_N, MAX_CELLS));                                              // cols * n would wrap

  // ---- transposition ----
  check_transpose(make(1, 1, {}));                                             // empty matrices
  check_transpose(make(5, 7, {}));
  check_transpose(make(1, 1, {{{0, 11}}}));                                    // a single entry
  check_transpose(make(4, 6, {{}, {}, {{3, 5}}, {}}));
  check_transpose(make(4, 3, {{{0, 1}}, {{0, 2}, {1, 9}}, {{1, 8}, {0, 3}}, {{0, 4}}}));       // a column holding every row; an empty last column
  check_transpose(make(3, 4, {{{2, 1}, {2, 2}, {0, 3}}, {{2, 4}}, {{1, 5}, {2, 6}, {2, 7}}}));  // duplicate (row, col) entries, unsorted columns within a row
  {
    std::vector<std::vector<std::pair<uint32_t, uint64_t>>> rows(40);         // a pseudo-random matrix, rows of 0..6 entries
    uint64_t x = 88172645463325252ull;
    for (auto& r : rows) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; for (uint64_t q = x % 7; q > 0; --q) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; r.push_back({(uint32_t)(x % 11), x}); } }
    check_transpose(make(40, 12, rows));
  }

  // ---- invalid inputs ----
  Csr g = make(4, 5, {{{0, 1}}, {{1, 2}, {4, 3}}, {}, {{2, 4}}});
  check_transpose(g);
  expect_invalid(g, nullptr, g.col.data(), g.val.data(), QAP_NO_ROW);                                  // null rowptr
  expect_invalid(g, g.rowptr.data(), nullptr, g.val.data(), QAP_NO_ROW);                               // entries without col / val
  expect_invalid(g, g.rowptr.data(), g.col.data(), nullptr, QAP_NO_ROW);
  { Csr b = g; b.rowptr[0] = 1; expect_invalid(b, b.rowptr.data(), b.col.data(), b.val.data(), QAP_NO_ROW); }      // rowptr[0] != 0
  { Csr b = g; b.rowptr[2] = 0; expect_invalid(b, b.rowptr.data(), b.col.data(), b.val.data(), 1); }               // a decreasing rowptr: row 1 ends before it starts
  { Csr b = g; b.rowptr[4] = 2; expect_invalid(b, b.rowptr.data(), b.col.data(), b.val.data(), 3); }
  { Csr b = g; b.col[2] = 5; expect_invalid(b, b.rowptr.data(), b.col.data(), b.val.data(), 1); }                  // col == cols, in row 1
  { Csr b = g; b.col[3] = 0xffffffffu; expect_invalid(b, b.rowptr.data(), b.col.data(), b.val.data(), 3); }
  { Csr b = g; b.col[0] = 5; b.col[3] = 9; expect_invalid(b, b.rowptr.data(), b.col.data(), b.val.data(), 0); }    // the first offending entry is reported
  { Csr b = make(2, 3, {}); b.rowptr = {0, 0, 0xffffffffull}; expect_invalid(b, b.rowptr.data(), nullptr, nullptr, QAP_NO_ROW); }     // too many entries, seen before col is read
  { Csr b = make(2, 3, {}); CHECK(qap_csr_valid(b.rowptr.data(), nullptr, nullptr, 2, 3, &b.n)); }                 // no entries: col and val may be null

  if (g_failed) { std::printf("%d checks failed\n", g_failed); return 1; }
  std::printf("qap_csc ok\n");
  return 0;
}
