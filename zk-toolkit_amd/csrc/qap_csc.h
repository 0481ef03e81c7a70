// R1CS matrix in the caller's CSR form (zkt_sparse_rows: one sparse row per constraint) -> validated, and transposed to the column-wise form the QAP build
// walks (zkt_qap.hip, k_qap_columns): for every wire its entries (constraint row, value), rows ascending.  Plain C++: pointers in, vectors out, no HIP, so
// tests/c/qap_csc_check.cpp exercises exactly this code under the host sanitizers.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <vector>

namespace zkt {

static constexpr size_t QAP_NO_ROW = ~(size_t)0;

// n constraints over `cols` wires within the limits of include/zkt.h (ZKT_QAP_MAX_N, ZKT_QAP_MAX_CELLS); the product cols * n is never formed
inline bool qap_dims_valid(size_t n, size_t cols, size_t max_n, size_t max_cells) { return n != 0 && cols != 0 && n <= max_n && cols <= max_cells / n; }

// true when the CSR is usable for n rows over `cols` columns: rowptr[0] == 0, rowptr non-decreasing, fewer than 2^32 entries, every col[k] < cols, and
// col / val present when there is an entry.  Otherwise false, with *bad_row = the constraint row of the first offending entry (a row whose end lies before
// its start; the row that holds a column index out of range), or QAP_NO_ROW where the fault has no row.
inline bool qap_csr_valid(const uint64_t* rowptr, const uint32_t* col, const uint64_t* val, size_t n, size_t cols, size_t* bad_row) {
  *bad_row = QAP_NO_ROW;
  if (!rowptr || rowptr[0] != 0) return false;
  for (size_t j = 0; j < n; ++j)
    if (rowptr[j + 1] < rowptr[j]) { *bad_row = j; return false; }
  const uint64_t nnz = rowptr[n];
  if (nnz >= 0xffffffffull) return false;
  if (nnz && (!col || !val)) return false;
  for (size_t j = 0; j < n; ++j)
    for (uint64_t k = rowptr[j]; k < rowptr[j + 1]; ++k)
      if (col[k] >= cols) { *bad_row = j; return false; }
  return true;
}

struct QapCsc {
  std::vector<uint32_t> colptr;      // cols + 1
  std::vector<uint32_t> row;         // nnz: the constraint row of every entry, ascending within a column (duplicates of one (row, col) stay adjacent, in input order)
  std::vector<uint64_t> val;         // nnz x 4 limbs, as given
};

// counting sort by column, stable in the row index.  The input must have passed qap_csr_valid.
inline void qap_csr_to_csc(const uint64_t* rowptr, const uint32_t* col, const uint64_t* val, size_t n, size_t cols, QapCsc& out) {
  const size_t nnz = (size_t)rowptr[n];
  out.colptr.assign(cols + 1, 0); out.row.resize(nnz); out.val.resize(nnz * 4);
  for (size_t k = 0; k < nnz; ++k) out.colptr[(size_t)col[k] + 1]++;
  for (size_t i = 0; i < cols; ++i) out.colptr[i + 1] += out.colptr[i];
  std::vector<uint32_t> cur(out.colptr.begin(), out.colptr.end() - 1);
  for (size_t j = 0; j < n; ++j)
    for (size_t k = (size_t)rowptr[j]; k < (size_t)rowptr[j + 1]; ++k) {
      const size_t d = cur[col[k]]++;
      out.row[d] = (uint32_t)j;
      memcpy(&out.val[d * 4], &val[k * 4], 32);
    }
}

}  // namespace zkt
