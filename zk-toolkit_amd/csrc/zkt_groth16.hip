// Groth16 on dense polynomials, orchestrated on the device (row a17 of SURVEY §8): src/zk/w_trusted_setup/groth16/zktoolkit_based/{crs.rs:49-146, prover.rs:96-147,
// verifier.rs:30-54}.  Random values the reference draws from OS entropy (alpha..x, r, s) are arguments.  Fr scalar algebra runs in small kernels here; every group operation
// goes through the batched kernels of zkt_group.hip / zkt_msm.hip / zkt_pairing.hip.  Host code only moves buffers and sequences launches (per-key caches: groth16_vk_cache.h).
#include <vector>
#include <cstring>
#include "fr_vec.h"
#include "host_abi.h"
#include "qap_handle.h"
#include "groth16_vk_cache.h"

namespace zkt {
// out[k] = sum_i a[i] * P[i*n + k]    (the combination sum_i a_i u_i of prover.rs:107-117, done in Fr first)
template <class C>
__global__ void __launch_bounds__(256) k_lincomb(const uint32_t* __restrict__ P, const uint32_t* __restrict__ a, size_t rows, size_t n, uint32_t* __restrict__ out) {
  size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  Fp<C> acc = fp_zero<C>();
  for (size_t i = 0; i < rows; ++i) acc = fp_add(acc, fp_mul(ld_fp<C>(a + i * C::N), ld_raw<C>(P + (i * n + k) * C::N)));   // aR * p * R^-1 = a p
  st_raw<C>(out + k * C::N, acc);
}
// CRS::new scalar stage (crs.rs:59-116): y_i = (beta u_i(x) + alpha v_i(x) + w_i(x)) / (gamma | delta), x^k, x^k t(x)/delta
__global__ void k_groth16_setup_scalars(const uint32_t* __restrict__ ue, const uint32_t* __restrict__ ve, const uint32_t* __restrict__ we,
                                        const uint32_t* __restrict__ trap /*alpha,beta,gamma,delta,x canonical*/, size_t n, size_t l, size_t m,
                                        uint32_t* __restrict__ y /*m+1*/, uint32_t* __restrict__ xpow /*n*/, uint32_t* __restrict__ xt /*n*/) {
  typedef FrC C;
  if (threadIdx.x || blockIdx.x) return;
  Fp<C> alpha = ld_fp<C>(trap), beta = ld_fp<C>(trap + 8), gamma = ld_fp<C>(trap + 16), delta = ld_fp<C>(trap + 24), x = ld_fp<C>(trap + 32);
  Fp<C> ginv = fp_inv(gamma), dinv = fp_inv(delta);
  for (size_t i = 0; i <= m; ++i) {
    Fp<C> s = fp_add(fp_add(fp_mul(beta, ld_raw<C>(ue + i * 8)), fp_mul(alpha, ld_raw<C>(ve + i * 8))), fp_canon32(ld_raw<C>(we + i * 8)));   // products reduce any 256-bit operand; the bare addend is reduced explicitly
    st_fp<C>(y + i * 8, fp_mul(s, i <= l ? ginv : dinv));
  }
  Fp<C> td = fp_mul(fr_t_at(x, n), dinv), xp = fp_one<C>();
  for (size_t k = 0; k < n; ++k) { st_fp<C>(xpow + k * 8, xp); st_fp<C>(xt + k * 8, fp_mul(xp, td)); xp = fp_mul(xp, x); }
}
}  // namespace zkt

using namespace zkt;

namespace {
// CRS::new (crs.rs:49-146), trapdoors injected.  hp: ui/vi/wi on the host, uploaded one after the other into one buffer; or dp: the same three arrays already on
// the device (a resident QAP), read in place.  (m+1) x n Fr coefficients each, low degree first.
int groth16_setup(zkt_groth16_crs* c, const uint64_t* const hp[3], const uint32_t* const dp[3],
                  const uint64_t* alpha, const uint64_t* beta, const uint64_t* gamma, const uint64_t* delta, const uint64_t* x) {
  const size_t n = c->n, l = c->l, m = c->m, rows = m + 1;
  hipStream_t s = nullptr;
  uint64_t trap[20]; memcpy(trap, alpha, 32); memcpy(trap + 4, beta, 32); memcpy(trap + 8, gamma, 32); memcpy(trap + 12, delta, 32); memcpy(trap + 16, x, 32);
  for (int k = 0; k < 5; ++k) if (fr_is_zero_mod_r(trap + 4 * k)) return ZKT_ERR_INV_ZERO;   // rand_elem(true): non-zero (crs.rs:59-63); the kernels reduce on load, so r and 2r are zero too
  Dev dP(hp ? rows * n * FRB : 0), dtrap(160), due(rows * FRB), dve(rows * FRB), dwe(rows * FRB), dy(rows * FRB), dxp(n * FRB), dxt(n * FRB);
  Dev dgen1(G1B), dgen2(G2B), dout1((rows + 2 * n + 3) * G1B), dout2((n + 3) * G2B), dgt(576), derr(8);
  int rc;
  if ((rc = up(dtrap, trap, 160, s)) || (rc = up(dgen1, &G1_GEN, G1B, s)) || (rc = up(dgen2, &G2_GEN, G2B, s))) return rc;
  Dev* evals[3] = {&due, &dve, &dwe};
  for (int k = 0; k < 3; ++k) {
    if (hp && (rc = up(dP, hp[k], rows * n * FRB, s))) return rc;
    fr_eval_rows(hp ? dP.w() : dp[k], rows, n, dtrap.w() + 32, evals[k]->w(), s);
  }
  hipLaunchKernelGGL(k_groth16_setup_scalars, dim3(1), dim3(64), 0, s, (const uint32_t*)due.w(), (const uint32_t*)dve.w(), (const uint32_t*)dwe.w(),
                     (const uint32_t*)dtrap.w(), n, l, m, dy.w(), dxp.w(), dxt.w());
  // fixed-base multiplications g * y (crs.rs:85-135): [uvw (m+1) | xi (n) | xt_by_delta (n) | alpha beta delta]
  uint32_t* o1 = dout1.w();
  HIPCHK(launch_generator_mul(G_G1, dgen1.w(), dy.w(), o1, rows, s));
  HIPCHK(launch_generator_mul(G_G1, dgen1.w(), dxp.w(), o1 + rows * 26, n, s));
  HIPCHK(launch_generator_mul(G_G1, dgen1.w(), dxt.w(), o1 + (rows + n) * 26, n, s));
  HIPCHK(launch_generator_mul(G_G1, dgen1.w(), dtrap.w(), o1 + (rows + 2 * n) * 26, 1, s));            // alpha
  HIPCHK(launch_generator_mul(G_G1, dgen1.w(), dtrap.w() + 8, o1 + (rows + 2 * n + 1) * 26, 1, s));    // beta
  HIPCHK(launch_generator_mul(G_G1, dgen1.w(), dtrap.w() + 24, o1 + (rows + 2 * n + 2) * 26, 1, s));   // delta
  uint32_t* o2 = dout2.w();
  HIPCHK(launch_generator_mul(G_G2, dgen2.w(), dxp.w(), o2, n, s));
  HIPCHK(launch_generator_mul(G_G2, dgen2.w(), dtrap.w() + 8, o2 + n * 50, 1, s));          // beta
  HIPCHK(launch_generator_mul(G_G2, dgen2.w(), dtrap.w() + 16, o2 + (n + 1) * 50, 1, s));   // gamma
  HIPCHK(launch_generator_mul(G_G2, dgen2.w(), dtrap.w() + 24, o2 + (n + 2) * 50, 1, s));   // delta
  unsigned long long noerr = NO_ERR; if ((rc = up(derr, &noerr, 8, s))) return rc;
  HIPCHK(launch_tate(o1 + (rows + 2 * n) * 26, o2 + n * 50, dgt.w(), 1, (unsigned long long*)derr.p, s));   // crs.rs:137-139
  if ((rc = down(c->g1_uvw_stmt, o1, (l + 1) * G1B, s)) || (rc = down(c->g1_uvw_wit, o1 + (l + 1) * 26, (m - l) * G1B, s)) ||
      (rc = down(c->g1_xi, o1 + rows * 26, n * G1B, s)) || (rc = down(c->g1_xt_by_delta, o1 + (rows + n) * 26, n * G1B, s)) ||
      (rc = down(c->g1_alpha, o1 + (rows + 2 * n) * 26, G1B, s)) || (rc = down(c->g1_beta, o1 + (rows + 2 * n + 1) * 26, G1B, s)) ||
      (rc = down(c->g1_delta, o1 + (rows + 2 * n + 2) * 26, G1B, s)) || (rc = down(c->g2_xi, o2, n * G2B, s)) ||
      (rc = down(c->g2_beta, o2 + n * 50, G2B, s)) || (rc = down(c->g2_gamma, o2 + (n + 1) * 50, G2B, s)) ||
      (rc = down(c->g2_delta, o2 + (n + 2) * 50, G2B, s)) || (rc = down(c->gt_alpha_beta, dgt.p, 576, s))) return rc;
  HIPCHK(hipStreamSynchronize(s));
  return ZKT_OK;
}
}  // namespace

extern "C" {
int zkt_groth16_setup(zkt_groth16_crs* c, const uint64_t* ui, const uint64_t* vi, const uint64_t* wi,
                      const uint64_t* alpha, const uint64_t* beta, const uint64_t* gamma, const uint64_t* delta, const uint64_t* x) {
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (!c || !ui || !vi || !wi || !alpha || !beta || !gamma || !delta || !x || c->n == 0 || c->l > c->m) return ZKT_ERR_SHAPE;
  const uint64_t* hp[3] = {ui, vi, wi};
  return groth16_setup(c, hp, nullptr, alpha, beta, gamma, delta, x);
}
// the same with ui, vi, wi read from a resident QAP (zkt_qap_create): nothing of size (m+1) x n is uploaded
int zkt_groth16_setup_resident(zkt_groth16_crs* c, const zkt_qap* q, const uint64_t* alpha, const uint64_t* beta, const uint64_t* gamma, const uint64_t* delta,
                               const uint64_t* x) {
  if (!c || !q || !alpha || !beta || !gamma || !delta || !x || c->n == 0 || c->l > c->m || q->n != c->n || q->cols != c->m + 1) return ZKT_ERR_SHAPE;
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  return groth16_setup(c, nullptr, q->m, alpha, beta, gamma, delta, x);
}

// Prover::prove (prover.rs:96-147), r and s injected.
// A = alpha + (sum_i a_i u_i)(x) G + r delta is one MSM over crs.g1.xi once the polynomials are combined in Fr
// (the reference does (m+1) MSMs and multiplies each by a_i — the same group element).
int zkt_groth16_prove(const zkt_groth16_crs* c, const uint64_t* ui, const uint64_t* vi, const uint64_t* wires,
                      const uint64_t* h, size_t h_len, const uint64_t* r, const uint64_t* s_, zkt_g1_affine* A, zkt_g2_affine* B, zkt_g1_affine* C) {
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (!c || !ui || !vi || !wires || !r || !s_ || !A || !B || !C || (h_len && !h) || h_len > c->n || c->l > c->m) return ZKT_ERR_SHAPE;   // h_len > n would index-panic (polynomial.rs:277-279)
  const size_t n = c->n, l = c->l, m = c->m, rows = m + 1, nw = m - l;
  hipStream_t s = nullptr;
  Dev dP(rows * n * FRB), dw(rows * FRB), dU(n * FRB), dV(n * FRB);
  int rc; if ((rc = up(dw, wires, rows * FRB, s))) return rc;
  if ((rc = up(dP, ui, rows * n * FRB, s))) return rc;
  hipLaunchKernelGGL(k_lincomb<FrC>, dim3(grid_blocks(n)), dim3(256), 0, s, (const uint32_t*)dP.w(), (const uint32_t*)dw.w(), rows, n, dU.w());
  if ((rc = up(dP, vi, rows * n * FRB, s))) return rc;
  hipLaunchKernelGGL(k_lincomb<FrC>, dim3(grid_blocks(n)), dim3(256), 0, s, (const uint32_t*)dP.w(), (const uint32_t*)dw.w(), rows, n, dV.w());
  std::vector<uint64_t> U(n * 4), V(n * 4);
  if ((rc = down(U.data(), dU.p, n * FRB, s)) || (rc = down(V.data(), dV.p, n * FRB, s))) return rc;
  HIPCHK(hipStreamSynchronize(s));
  zkt_g1_affine sumA, sumB1, sumW, ht; zkt_g2_affine sumB;
  if ((rc = zkt_g1_msm(c->g1_xi, U.data(), n, &sumA)) || (rc = zkt_g2_msm(c->g2_xi, V.data(), n, &sumB)) || (rc = zkt_g1_msm(c->g1_xi, V.data(), n, &sumB1))) return rc;
  if ((rc = zkt_g1_msm(c->g1_uvw_wit, wires + (l + 1) * 4, nw, &sumW)) || (rc = zkt_g1_msm(c->g1_xt_by_delta, h, h_len, &ht))) return rc;
  // the seven single scalar multiplications and the final sums (prover.rs:118-140)
  zkt_g1_affine dr, ds, As, Br, drs, t1, t2;
  if ((rc = zkt_g1_mul_batch(c->g1_delta, r, 4, &dr, 1)) || (rc = zkt_g1_mul_batch(c->g1_delta, s_, 4, &ds, 1))) return rc;
  zkt_g2_affine d2s; if ((rc = zkt_g2_mul_batch(c->g2_delta, s_, 4, &d2s, 1))) return rc;
  if ((rc = zkt_g1_add_batch(c->g1_alpha, &sumA, &t1, 1)) || (rc = zkt_g1_add_batch(&t1, &dr, A, 1))) return rc;               // A
  zkt_g2_affine t3; if ((rc = zkt_g2_add_batch(c->g2_beta, &sumB, &t3, 1)) || (rc = zkt_g2_add_batch(&t3, &d2s, B, 1))) return rc;   // B
  zkt_g1_affine B1; if ((rc = zkt_g1_add_batch(c->g1_beta, &sumB1, &t1, 1)) || (rc = zkt_g1_add_batch(&t1, &ds, &B1, 1))) return rc; // B_g1
  if ((rc = zkt_g1_mul_batch(A, s_, 4, &As, 1)) || (rc = zkt_g1_mul_batch(&B1, r, 4, &Br, 1)) || (rc = zkt_g1_mul_batch(&dr, s_, 4, &drs, 1))) return rc;
  zkt_g1_affine ndrs; if ((rc = zkt_g1_neg_batch(&drs, &ndrs, 1))) return rc;
  if ((rc = zkt_g1_add_batch(&sumW, &ht, &t1, 1)) || (rc = zkt_g1_add_batch(&t1, &As, &t2, 1)) || (rc = zkt_g1_add_batch(&t2, &Br, &t1, 1)) ||
      (rc = zkt_g1_add_batch(&t1, &ndrs, C, 1))) return rc;                                                                        // C
  return ZKT_OK;
}

// Verifier::verify (verifier.rs:30-54) for a batch of proofs against one CRS, one proof per lane: the three pairings of a
// proof share one Miller squaring chain and one final exponentiation.  stmt_wires: n_proofs x n_stmt Fr.
// ok[i] = 1 accept / 0 reject.  Returns ZKT_OK, or ZKT_ERR_INFINITY (+index) if some pairing argument is the point at infinity.
int zkt_groth16_verify_batch(const zkt_groth16_crs* c, const zkt_g1_affine* A, const zkt_g2_affine* B, const zkt_g1_affine* C,
                             const uint64_t* stmt_wires, size_t n_stmt, size_t n_proofs, uint32_t* ok) {
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (!c || !A || !B || !C || !ok || (n_stmt && !stmt_wires) || n_stmt > c->l + 1) return ZKT_ERR_SHAPE;
  if (n_proofs == 0) return ZKT_OK;
  hipStream_t s = nullptr;
  const bool P = true;       // pooled: everything below runs on the legacy stream
  Dev dA(n_proofs * G1B, P), dB(n_proofs * G2B, P), dC(n_proofs * G1B, P), dU((n_stmt ? n_stmt : 1) * G1B, P), dW((n_proofs * n_stmt ? n_proofs * n_stmt : 1) * FRB, P),
      dg(G2B, P), dd(G2B, P), dab(576, P), dok(n_proofs * 4, P), derr(8, P);
  int rc;
  if ((rc = up(dA, A, n_proofs * G1B, s)) || (rc = up(dB, B, n_proofs * G2B, s)) || (rc = up(dC, C, n_proofs * G1B, s)) ||
      (rc = up(dU, c->g1_uvw_stmt, n_stmt * G1B, s)) || (rc = up(dW, stmt_wires, n_proofs * n_stmt * FRB, s)) ||
      (rc = up(dg, c->g2_gamma, G2B, s)) || (rc = up(dd, c->g2_delta, G2B, s)) || (rc = up(dab, c->gt_alpha_beta, 576, s))) return rc;
  unsigned long long noerr = NO_ERR; if ((rc = up(derr, &noerr, 8, s))) return rc;
  if (!dok.p) return ZKT_ERR_DEVICE;
  if (n_stmt >= 1 && n_stmt <= 12 && n_proofs * 3 <= dproduct_limit()) {      // few proofs: one proof per three lane groups (zkt_dpairing.hip), ~15 ms instead of ~105 ms
    Dev dtmp(n_stmt * n_proofs * G1B, P), dS(n_proofs * G1B, P);
    if (!dtmp.p || !dS.p) return ZKT_ERR_DEVICE;
    std::shared_ptr<void> akey;                                                                   // null: a key the 63-step loop may not serve, or one whose entry is not there yet -> the 127-step loop against alpha_beta
    AteBuild build;
    if (ate_key_lookup(c, n_stmt, &akey) == ATE_ABSENT) build.begin(c, n_stmt, dU.w(), dg.w(), dd.w(), s);      // first sight: the entry is built beside this call
    const std::shared_ptr<void> tabs = stmt_tables_for(c->g1_uvw_stmt, n_stmt, dU.w(), s);     // held until the synchronisation below
    build.tables((const uint32_t*)tabs.get());
    const uint32_t* ate_target = akey ? (const uint32_t*)akey.get() + ATE_KEY_TARGET : nullptr;
    HIPCHK(launch_groth16_verify_small(dA.w(), dB.w(), dC.w(), dU.w(), (const uint32_t*)tabs.get(), dW.w(), (int)n_stmt, dg.w(), dd.w(), dab.w(), dtmp.w(), dS.w(), dok.w(), n_proofs, (unsigned long long*)derr.p, s, ate_target));
    return finish_verdicts(ok, dok.p, n_proofs, derr.p, s);
  }
  const std::shared_ptr<void> akey = ate_key_now(c, n_stmt, dU.w(), dg.w(), dd.w(), s);      // held until the synchronisation below; null: the value-comparing kernels
  HIPCHK(launch_groth16_verify(dA.w(), dB.w(), dC.w(), dU.w(), dW.w(), (int)n_stmt, dg.w(), dd.w(), dab.w(), dok.w(), n_proofs, (unsigned long long*)derr.p, s, (const uint32_t*)akey.get()));
  return finish_verdicts(ok, dok.p, n_proofs, derr.p, s);
}
// What a verifier that KNOWS its key calls once: the statement points' fixed-base tables and the key's entry for the 63-step loop (line tables of gamma and delta,
// the ate counterpart of alpha_beta, 8-bit statement tables; ~20 ms) are built now instead of at the second verification against the key (verifier.rs:30-54 builds
// nothing per key; crs.rs:137-139 computes alpha_beta once).  Returns ZKT_OK whether or not the key qualifies for the 63-step loop (a key carrying a point outside its
// group, or an alpha_beta that is not tate(alpha, beta), keeps the value-comparing kernels — decisions are the same either way).
int zkt_groth16_vk_prepare(const zkt_groth16_crs* c, size_t n_stmt) {
  if (zkt_internal_ready() != ZKT_OK) return ZKT_ERR_DEVICE;
  if (!c || n_stmt > c->l + 1) return ZKT_ERR_SHAPE;
  if (n_stmt < 1 || n_stmt > 12) return ZKT_OK;      // such statements are summed in the lanes: nothing to prepare
  hipStream_t s = nullptr;
  Dev dU(n_stmt * G1B, true), dg(G2B, true), dd(G2B, true);
  int rc;
  if ((rc = up(dU, c->g1_uvw_stmt, n_stmt * G1B, s)) || (rc = up(dg, c->g2_gamma, G2B, s)) || (rc = up(dd, c->g2_delta, G2B, s))) return rc;
  const std::shared_ptr<void> akey = ate_key_now(c, n_stmt, dU.w(), dg.w(), dd.w(), s);      // builds the statement points' 16^k tables on its way
  const std::shared_ptr<void> tabs = stmt_tables_for(c->g1_uvw_stmt, n_stmt, dU.w(), s);
  HIPCHK(hipStreamSynchronize(s));
  return ZKT_OK;
}
// single proof: 1 = accept, 0 = reject, negative = -status (a pairing argument at infinity panics in the reference)
int zkt_groth16_verify(const zkt_groth16_crs* c, const zkt_g1_affine* A, const zkt_g2_affine* B, const zkt_g1_affine* C,
                       const uint64_t* stmt_wires, size_t n_stmt) {
  uint32_t ok = 0;
  int rc = zkt_groth16_verify_batch(c, A, B, C, stmt_wires, n_stmt, 1, &ok);
  if (rc != ZKT_OK) return -rc;
  return (int)ok;
}
}  // extern "C"
