// R1CS -> QAP on the device: the reference's QAP::build (qap/qap.rs:137-203), which interpolates every wire's column of A, B and C over the domain {1..n}
// through build_polynomial (qap.rs:33-97, n polynomial products per Lagrange basis polynomial).  The interpolant of degree < n through n points is unique, so
// the same n coefficients per wire come out of
//   t(x)   = prod_{i=1..n} (x - i)                                    build_t_dev (zkt_poly.hip)
//   q_j(x) = t(x) / (x - j), n coefficients                           synthetic division: c = t[k] + c j, q_j[k-1] = c for k = n .. 1   (k_qap_basis)
//   w_j    = 1 / t'(j) = (-1)^(n-j) / ((j-1)! (n-j)!)                 factorials by two prefix products and ONE inversion              (k_qap_weights)
//   u_i    = sum_j M[j][i] w_j q_j                                     one lane per coefficient of every wire                           (k_qap_columns)
// with exact Fr arithmetic throughout (Montgomery inside, canonical at the caller's boundary).
// The basis table is laid out [j][k] (row j = q_j): k_qap_columns, which reads nnz * n of its elements, then reads consecutive lanes' elements from
// consecutive addresses; k_qap_basis pays for it with 32-byte stores n elements apart.  profiles/qap_build_timing.md has the two kernels' measured shares
// (tools/diag/qap_build_timing.py makes them); tests/qap_build_model.py restates the algorithm in python integers.
// A lane of k_qap_columns is one (wire, coefficient) cell of the flat cols x n output, so short polynomials share a block and no grid dimension grows with cols.
#include <vector>
#include <memory>
#include <cstring>
#include "fr_vec.h"
#include "zkt_internal.h"
#include "../../include/zkt.h"
#include "host_abi.h"
#include "fr_pool.h"
#include "qap_csc.h"
#include "qap_handle.h"

namespace zkt {
namespace {
typedef FrC C;
static constexpr int QAP_TPB = 256;          // lanes per block of k_qap_basis (one basis row each) and of k_qap_columns (one output cell each)

// f[i] = max(i, 1) (prefix product: i!) and g[i] = max(n - 1 - i, 1) (prefix product: (n-1)! / (n-2-i)! for i <= n - 2), i < n
__global__ void __launch_bounds__(256) k_qap_iota(uint32_t* __restrict__ f, uint32_t* __restrict__ g, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; if (i >= n) return;
  stm4(f + i * FW, fr_small(i ? (uint32_t)i : 1u));
  stm4(g + i * FW, fr_small(n - 1 - i ? (uint32_t)(n - 1 - i) : 1u));
}
// *out = 1 / *in, one lane ((n-1)! is never zero: n <= ZKT_QAP_MAX_N is far below r)
__global__ void k_qap_inv1(const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  if (threadIdx.x || blockIdx.x) return;
  stm4(out, fp_inv(ldm4(in)));
}
// 1 / k! = (1 / (n-1)!) * (n-1)! / k!,  k < n
__device__ inline Fr qap_inv_fact(const uint32_t* __restrict__ g, const Fr& inv_top, size_t n, size_t k) {
  return k == n - 1 ? inv_top : fp_mul(inv_top, ldm4(g + (n - 2 - k) * FW));
}
// w[j-1] = (-1)^(n-j) / ((j-1)! (n-j)!), j = 1..n
__global__ void __launch_bounds__(256) k_qap_weights(const uint32_t* __restrict__ g, const uint32_t* __restrict__ inv_top, size_t n, uint32_t* __restrict__ w) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; if (i >= n) return;
  const Fr it = ldm4(inv_top);
  Fr c = fp_mul(qap_inv_fact(g, it, n, i), qap_inv_fact(g, it, n, n - 1 - i));
  if ((n - 1 - i) & 1) c = fp_neg(c);
  stm4(w + i * FW, c);
}
// c[e] = val[e] * w[row[e]] for every stored entry (val in the caller's layout: any 256-bit integer, reduced on load)
__global__ void __launch_bounds__(256) k_qap_scale(const uint32_t* __restrict__ val, const uint32_t* __restrict__ row, const uint32_t* __restrict__ w,
                                                   size_t nnz, uint32_t* __restrict__ c) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; if (e >= nnz) return;
  stm4(c + e * FW, fp_mul(ldx<true>(val + e * FW), ldm4(w + (size_t)row[e] * FW)));
}
// basis[j][0 .. n) = q_{j+1} = t / (x - (j + 1)): lanes over j, the uniform t[k] read once per step
__global__ void __launch_bounds__(QAP_TPB) k_qap_basis(const uint32_t* __restrict__ t, size_t n, uint32_t* __restrict__ basis) {
  const size_t j = (size_t)blockIdx.x * QAP_TPB + threadIdx.x; if (j >= n) return;
  const Fr x = fr_small((uint32_t)(j + 1));
  uint32_t* q = basis + j * n * FW;
  Fr c = fp_zero<C>();
  for (size_t k = n; k >= 1; --k) {
    c = fp_add(ldm4(t + k * FW), fp_mul(c, x));
    stm4(q + (k - 1) * FW, c);
  }
}
// out[m][i][k] = sum over the entries e of column i of matrix m of c[e] * basis[row[e]][k], m = blockIdx.y; EVERY cell is stored (an empty column: zeros),
// in the caller's layout.  Entries with the same (row, col) add.
struct QapMats { const uint32_t* colptr[3]; const uint32_t* row[3]; const uint32_t* c[3]; uint32_t* out[3]; };
__global__ void __launch_bounds__(QAP_TPB) k_qap_columns(QapMats a, const uint32_t* __restrict__ basis, size_t n, size_t cells) {
  const size_t cell = (size_t)blockIdx.x * QAP_TPB + threadIdx.x; if (cell >= cells) return;
  const size_t i = cell / n, k = cell - i * n;
  const int m = blockIdx.y;
  const uint32_t* row = a.row[m]; const uint32_t* c = a.c[m];
  Fr acc = fp_zero<C>();
  for (uint32_t e = a.colptr[m][i], end = a.colptr[m][i + 1]; e < end; ++e)
    acc = fp_add(acc, fp_mul(ldm4(c + (size_t)e * FW), ldm4(basis + ((size_t)row[e] * n + k) * FW)));
  stx<true>(a.out[m] + cell * FW, acc);
}

thread_local float t_basis_ms = 0.f, t_columns_ms = 0.f;

struct Events {
  hipEvent_t e[3] = {nullptr, nullptr, nullptr};
  int create() { for (hipEvent_t& x : e) HIPCHK(hipEventCreate(&x)); return ZKT_OK; }
  ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

bool qap_args_valid(size_t n, size_t cols, const zkt_sparse_rows* const M[3]) {
  if (!M[0] || !M[1] || !M[2]) return false;
  if (!qap_dims_valid(n, cols, ZKT_QAP_MAX_N, ZKT_QAP_MAX_CELLS)) return false;
  for (int k = 0; k < 3; ++k) {
    size_t bad;
    if (!qap_csr_valid(M[k]->rowptr, M[k]->col, M[k]->val, n, cols, &bad)) { if (bad != QAP_NO_ROW) zkt_internal_set_error_index(bad); return false; }
  }
  return true;
}

// the arguments have passed qap_args_valid and the library is ready
int qap_create(size_t n, size_t cols, const zkt_sparse_rows* const M[3], zkt_qap** out) {
  hipStream_t s = nullptr;
  const size_t cells = cols * n;
  std::unique_ptr<zkt_qap> q(new zkt_qap);
  q->n = n; q->cols = cols;
  for (int k = 0; k < 3; ++k) { void* p = nullptr; if (hipMalloc(&p, cells * FRB) != hipSuccess) { (void)hipGetLastError(); return ZKT_ERR_DEVICE; } q->m[k] = (uint32_t*)p; }
  Events ev; ZCHK(ev.create());
  Pool pool(s);
  // column-wise copies of the three matrices and their scaled entries
  QapCsc csc[3]; Dev colptr[3], row[3];
  QapMats a;
  PGET(w, pool, n); PGET(F, pool, n); PGET(G, pool, n); PGET(inv_top, pool, 1);
  hipLaunchKernelGGL(k_qap_iota, dim3(grid_blocks(n)), dim3(256), 0, s, F, G, n);
  ZCHK(fr_scan_mul(F, F, n, s)); ZCHK(fr_scan_mul(G, G, n, s));
  hipLaunchKernelGGL(k_qap_inv1, dim3(1), dim3(64), 0, s, (const uint32_t*)(F + (n - 1) * FW), inv_top);
  hipLaunchKernelGGL(k_qap_weights, dim3(grid_blocks(n)), dim3(256), 0, s, (const uint32_t*)G, (const uint32_t*)inv_top, n, w);
  for (int k = 0; k < 3; ++k) {
    qap_csr_to_csc(M[k]->rowptr, M[k]->col, M[k]->val, n, cols, csc[k]);
    const size_t nnz = csc[k].row.size();
    ZCHK(colptr[k].alloc((cols + 1) * 4, true)); ZCHK(row[k].alloc(nnz * 4, true));
    ZCHK(up(colptr[k], csc[k].colptr.data(), (cols + 1) * 4, s)); ZCHK(up(row[k], csc[k].row.data(), nnz * 4, s));
    PGET(val, pool, nnz); PGET(c, pool, nnz);
    if (nnz) {
      HIPCHK(hipMemcpyAsync(val, csc[k].val.data(), nnz * FRB, hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(k_qap_scale, dim3(grid_blocks(nnz)), dim3(256), 0, s, (const uint32_t*)val, (const uint32_t*)row[k].w(), (const uint32_t*)w, nnz, c);
    }
    a.colptr[k] = colptr[k].w(); a.row[k] = row[k].w(); a.c[k] = c; a.out[k] = q->m[k];
  }
  PGET(T, pool, n + 1); PGET(basis, pool, n * n);
  ZCHK(build_t_dev(pool, n, T));
  HIPCHK(hipEventRecord(ev.e[0], s));
  hipLaunchKernelGGL(k_qap_basis, dim3(grid_blocks(n, QAP_TPB)), dim3(QAP_TPB), 0, s, (const uint32_t*)T, n, basis);
  HIPCHK(hipEventRecord(ev.e[1], s));
  hipLaunchKernelGGL(k_qap_columns, dim3(grid_blocks(cells, QAP_TPB), 3), dim3(QAP_TPB), 0, s, a, (const uint32_t*)basis, n, cells);
  HIPCHK(hipEventRecord(ev.e[2], s));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s));            // the host vectors of `csc` and the pooled buffers end with this frame
  HIPCHK(hipEventElapsedTime(&t_basis_ms, ev.e[0], ev.e[1])); HIPCHK(hipEventElapsedTime(&t_columns_ms, ev.e[1], ev.e[2]));
  *out = q.release();
  return ZKT_OK;
}

int qap_download(const zkt_qap* q, uint64_t* const dst[3]) {
  const size_t bytes = q->cols * q->n * FRB;
  for (int k = 0; k < 3; ++k) if (dst[k]) HIPCHK(hipMemcpyAsync(dst[k], q->m[k], bytes, hipMemcpyDeviceToHost, nullptr));
  HIPCHK(hipStreamSynchronize(nullptr));
  return ZKT_OK;
}
}  // namespace
}  // namespace zkt

using namespace zkt;

extern "C" {

// QAP::build (qap.rs:137-203), kept on the device
int zkt_qap_create(size_t n, size_t cols, const zkt_sparse_rows* A, const zkt_sparse_rows* B, const zkt_sparse_rows* Cm, zkt_qap** out) {
  const zkt_sparse_rows* M[3] = {A, B, Cm};
  if (!out || !qap_args_valid(n, cols, M)) return ZKT_ERR_SHAPE;
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  return qap_create(n, cols, M, out);
}
int zkt_qap_download(const zkt_qap* q, uint64_t* ui, uint64_t* vi, uint64_t* wi) {
  if (!q) return ZKT_ERR_SHAPE;
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  uint64_t* dst[3] = {ui, vi, wi};
  return qap_download(q, dst);
}
void zkt_qap_free(zkt_qap* q) {
  if (!q) return;
  (void)zkt_internal_ready();                  // the calling thread's device becomes the library's
  delete q;
}
// QAP::build with the three arrays returned to the host
int zkt_qap_build(size_t n, size_t cols, const zkt_sparse_rows* A, const zkt_sparse_rows* B, const zkt_sparse_rows* Cm, uint64_t* ui, uint64_t* vi, uint64_t* wi) {
  const zkt_sparse_rows* M[3] = {A, B, Cm};
  if (!ui || !vi || !wi || !qap_args_valid(n, cols, M)) return ZKT_ERR_SHAPE;
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  zkt_qap* q = nullptr;
  ZCHK(qap_create(n, cols, M, &q));
  std::unique_ptr<zkt_qap> own(q);
  uint64_t* dst[3] = {ui, vi, wi};
  return qap_download(q, dst);
}
// the time the last zkt_qap_create / zkt_qap_build of this thread spent in k_qap_basis and in k_qap_columns (events around the two launches)
void zkt_qap_last_build_ms(float* basis_ms, float* columns_ms) {
  if (basis_ms) *basis_ms = t_basis_ms;
  if (columns_ms) *columns_ms = t_columns_ms;
}

}  // extern "C"
