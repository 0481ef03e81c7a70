//! QAP (zk/w_trusted_setup/qap/qap.rs): `QAP::build` (:137-203, build_polynomial :33-97) interpolates every wire's column of the R1CS over the domain {1..n}
//! on the device and keeps the three arrays there (zkt_qap_create); `QAP::is_valid` (:205-217) is the quotient of build_p (:99-112) by build_t (:115-135) read
//! from the handle (zkt_qap_quotient_resident).  `groth16::CRS::new_from_qap` and `groth16::prove_from_qap` consume the same handle, so R1CS -> CRS -> proof in
//! coefficient form moves no (m+1) x n array between host and device.  The reference names its three families vi, wi, yi; Groth16 calls them ui, vi, wi.
//! `polynomials()` brings them back (what `pinocchio::CRS` takes).  The reference's R1CS (equation parser, gates, templates) stays with the caller: the
//! constraint matrices arrive as `groth16::SparseRows`, one sparse row per constraint.
use crate::ffi::{self, zkt_sparse_rows};
use crate::field::{Bls12R, Fr, PrimeField, SparseVec};
use crate::groth16::SparseRows;
use crate::polynomial::Polynomial;
use crate::{check, init};

/// constraints and wires one QAP may have (ZKT_QAP_MAX_N, ZKT_QAP_MAX_CELLS of include/zkt.h)
pub const QAP_MAX_N: usize = 8192;
pub const QAP_MAX_CELLS: usize = 1 << 26;

/// qap.rs:18-25, resident: `num_constraints` polynomial coefficients per witness value in each of vi, wi, yi
pub struct QAP { h: *mut ffi::zkt_qap, pub f: PrimeField<Bls12R>, pub num_constraints: usize, pub num_witness_values: usize }
unsafe impl Send for QAP {}

impl QAP {
    /// qap.rs:137-203 on the constraint matrices a, b, c of `r1cs.to_constraint_matrices()` (:154): `num_witness_values` columns each
    pub fn build(f: &PrimeField<Bls12R>, num_witness_values: usize, a: &SparseRows, b: &SparseRows, c: &SparseRows) -> QAP {
        init();
        let n = a.rowptr.len() - 1;
        assert!(b.rowptr.len() == n + 1 && c.rowptr.len() == n + 1, "the three matrices have one row per constraint");
        let vals: Vec<Vec<u64>> = [a, b, c].iter().map(|r| Fr::flatten(&r.val)).collect();
        let rows: Vec<zkt_sparse_rows> = [a, b, c].iter().zip(vals.iter()).map(|(r, v)| zkt_sparse_rows { rowptr: r.rowptr.as_ptr(), col: r.col.as_ptr(), val: v.as_ptr() }).collect();
        let mut h = std::ptr::null_mut();
        check(unsafe { ffi::zkt_qap_create(n, num_witness_values, &rows[0], &rows[1], &rows[2], &mut h) });
        QAP { h, f: f.clone(), num_constraints: n, num_witness_values }
    }
    /// qap.rs:205-217: t divides p.  (`num_constraints` is the reference's second argument; the handle knows it.)
    pub fn is_valid(&self, witness: &SparseVec<Bls12R>, num_constraints: usize) -> bool {
        assert!(num_constraints == self.num_constraints, "the QAP was built over {} constraints", self.num_constraints);
        self.quotient(&witness.to_dense()).is_some()
    }
    /// h = p / t of Prover::new (groth16/zktoolkit_based/prover.rs:64-71), or None where the reference panics with "p should be divisible by t"
    pub fn quotient(&self, wires: &[Fr]) -> Option<Polynomial> {
        assert!(wires.len() == self.num_witness_values, "one value per wire");
        let n = self.num_constraints;
        let a = Fr::flatten(wires);
        let mut h = vec![0u64; (n - 1).max(1) * 4];
        let rc = unsafe { ffi::zkt_qap_quotient_resident(self.h, a.as_ptr(), h.as_mut_ptr()) };
        if rc == ffi::ZKT_ERR_REMAINDER { return None; }
        check(rc);
        Some(if n == 1 { Polynomial::zero() } else { Polynomial { coeffs: Fr::unflatten(&h) } })
    }
    /// the three families as the reference holds them (qap.rs:21-23), num_constraints coefficients each, low degree first, not normalised
    pub fn polynomials(&self) -> (Vec<Vec<Fr>>, Vec<Vec<Fr>>, Vec<Vec<Fr>>) {
        let (n, cols) = (self.num_constraints, self.num_witness_values);
        let (mut u, mut v, mut w) = (vec![0u64; cols * n * 4], vec![0u64; cols * n * 4], vec![0u64; cols * n * 4]);
        check(unsafe { ffi::zkt_qap_download(self.h, u.as_mut_ptr(), v.as_mut_ptr(), w.as_mut_ptr()) });
        let split = |x: &Vec<u64>| -> Vec<Vec<Fr>> { x.chunks(n * 4).map(Fr::unflatten).collect() };
        (split(&u), split(&v), split(&w))
    }
    pub fn raw(&self) -> *const ffi::zkt_qap { self.h }
}
impl Drop for QAP { fn drop(&mut self) { unsafe { ffi::zkt_qap_free(self.h) } } }
