//! Polynomial (building_block/field/polynomial.rs): multiply_by / divide_by / eval_at / eval_from_1_to_n (:173-262) on the device's dense Fr engine
//! (zkt_fr_poly_*), and eval_with_g1_hidings / eval_with_g2_hidings (:271-293): sum_i coeffs[i] * powers[i] — the MSM.
//! `build_t` and `quotient` are QAP::build_t and the p / t of Prover::new (qap/qap.rs:99-135, groth16/zktoolkit_based/prover.rs:64-71).
//! Resident base sets (`G1Bases`, `G2Bases`) are the analogue of a CRS that is uploaded once and reused by every proof.
use crate::ffi;
use crate::field::{Bls12R, Fr, PrimeField, SparseVec};
use crate::points::{G1Point, G2Point};
use crate::{check, init};

#[derive(Clone, Debug)]
pub struct Polynomial { pub coeffs: Vec<Fr> } // polynomial.rs: coefficients, low degree first

/// polynomial.rs:113-116
#[derive(Clone, Debug)]
pub enum DivResult {
    Quotient(Polynomial),
    QuotientRemainder((Polynomial, Polynomial)),
}

impl Polynomial {
    /// polynomial.rs:119-127: trailing zero coefficients are trimmed, the 0th is always kept (normalize, :139-152)
    pub fn new(coeffs: &[Fr]) -> Self {
        if coeffs.is_empty() { panic!("coeffs is empty"); }
        let mut len = coeffs.len();
        while len > 1 && coeffs[len - 1].is_zero() { len -= 1; }
        Polynomial { coeffs: coeffs[..len].to_vec() }
    }
    pub fn zero() -> Self { Polynomial { coeffs: vec![Fr::new(&0u8)] } } // :129-132
    pub fn is_zero(&self) -> bool { self.coeffs.len() == 1 && self.coeffs[0].is_zero() } // :134-136
    pub fn len(&self) -> usize { self.coeffs.len() }
    /// polynomial.rs:173-190 — len() + rhs.len() - 1 coefficients, not normalised
    pub fn multiply_by(&self, rhs: &Polynomial) -> Polynomial {
        init();
        let (a, b) = (Fr::flatten(&self.coeffs), Fr::flatten(&rhs.coeffs));
        let mut out = vec![0u64; (self.len() + rhs.len() - 1) * 4];
        check(unsafe { ffi::zkt_fr_poly_mul(a.as_ptr(), self.len(), b.as_ptr(), rhs.len(), out.as_mut_ptr()) });
        Polynomial { coeffs: Fr::unflatten(&out) }
    }
    /// polynomial.rs:204-238 — the quotient keeps len() - rhs.len() + 1 coefficients; the remainder is normalised
    pub fn divide_by(&self, rhs: &Polynomial) -> DivResult {
        init();
        assert!(self.len() >= rhs.len(), "attempt to subtract with overflow");
        assert!(!rhs.coeffs[rhs.len() - 1].is_zero(), "found zero coeff at highest index. use Polynomial constructor");
        let (a, b) = (Fr::flatten(&self.coeffs), Fr::flatten(&rhs.coeffs));
        let mut q = vec![0u64; (self.len() - rhs.len() + 1) * 4];
        let mut rem = vec![0u64; (rhs.len() - 1).max(1) * 4];
        let mut rem_len = 0usize;
        check(unsafe { ffi::zkt_fr_poly_divrem(a.as_ptr(), self.len(), b.as_ptr(), rhs.len(), q.as_mut_ptr(), rem.as_mut_ptr(), &mut rem_len) });
        let quotient = Polynomial { coeffs: Fr::unflatten(&q) };
        if rem_len == 0 { DivResult::Quotient(quotient) } else { DivResult::QuotientRemainder((quotient, Polynomial { coeffs: Fr::unflatten(&rem[..rem_len * 4]) })) }
    }
    /// one call for many points (the batch form of eval_at)
    pub fn eval_batch(&self, xs: &[Fr]) -> Vec<Fr> {
        init();
        let (c, x) = (Fr::flatten(&self.coeffs), Fr::flatten(xs));
        let mut out = vec![0u64; xs.len() * 4];
        check(unsafe { ffi::zkt_fr_poly_eval_batch(c.as_ptr(), self.len(), x.as_ptr(), xs.len(), out.as_mut_ptr()) });
        Fr::unflatten(&out)
    }
    /// polynomial.rs:240-249
    pub fn eval_at(&self, x: &Fr) -> Fr { self.eval_batch(std::slice::from_ref(x)).pop().unwrap() }
    /// polynomial.rs:251-262 — the values at 1..n, at the indices 0..n-1 of a SparseVec of size n
    pub fn eval_from_1_to_n(&self, n: &Fr) -> SparseVec<Bls12R> {
        let size = n.limbs[0] as usize;
        assert!(n.limbs[1..].iter().all(|w| *w == 0), "n does not fit the engine's batch size");
        let xs: Vec<Fr> = (1..=size as u64).map(|i| Fr::new(&i)).collect();
        let mut vec = SparseVec::new(size);
        for (i, v) in self.eval_batch(&xs).iter().enumerate() { vec.set(i, v); }
        vec
    }
    /// QAP::build_t qap.rs:115-135: prod_{i=1..n} (x - i)
    pub fn build_t(_f: &PrimeField<Bls12R>, num_constraints: usize) -> Polynomial {
        init();
        let mut out = vec![0u64; (num_constraints + 1) * 4];
        check(unsafe { ffi::zkt_qap_build_t(num_constraints, out.as_mut_ptr()) });
        Polynomial { coeffs: Fr::unflatten(&out) }
    }
    /// h = ((sum a_i u_i) (sum a_i v_i) - sum a_i w_i) / t (qap.rs:99-112, prover.rs:64-71): ui, vi, wi have one polynomial of n coefficients per wire.
    /// Panics with the reference's "p should be divisible by t" when the witness does not satisfy the constraints.
    pub fn quotient(ui: &[Vec<Fr>], vi: &[Vec<Fr>], wi: &[Vec<Fr>], wires: &[Fr]) -> Polynomial {
        init();
        let (rows, n) = (wires.len(), ui[0].len());
        let flat = |m: &[Vec<Fr>]| -> Vec<u64> { assert!(m.len() == rows && m.iter().all(|p| p.len() == n)); m.iter().flat_map(|p| Fr::flatten(p)).collect() };
        let (u, v, w, a) = (flat(ui), flat(vi), flat(wi), Fr::flatten(wires));
        let mut h = vec![0u64; (n - 1).max(1) * 4];
        let rc = unsafe { ffi::zkt_qap_quotient(u.as_ptr(), v.as_ptr(), w.as_ptr(), rows, n, a.as_ptr(), h.as_mut_ptr()) };
        if rc == ffi::ZKT_ERR_REMAINDER { panic!("p should be divisible by t"); }
        check(rc);
        if n == 1 { Polynomial::zero() } else { Polynomial { coeffs: Fr::unflatten(&h) } }
    }
    /// polynomial.rs:271-281 — panics if there are fewer powers than coefficients, as the reference's index does (:277-279)
    #[allow(non_snake_case)]
    pub fn eval_with_g1_hidings(&self, powers: &[G1Point]) -> G1Point {
        init();
        let n = self.coeffs.len();
        assert!(powers.len() >= n, "index out of bounds: the len is {} but the index is {}", powers.len(), powers.len());
        let p: Vec<ffi::zkt_g1_affine> = powers[..n].iter().map(|x| x.to_raw()).collect();
        let k = Fr::flatten(&self.coeffs);
        let mut out = G1Point::zero_raw();
        check(unsafe { ffi::zkt_g1_msm(p.as_ptr(), k.as_ptr(), n, &mut out) });
        G1Point::from_raw(&out)
    }
    /// polynomial.rs:283-293
    #[allow(non_snake_case)]
    pub fn eval_with_g2_hidings(&self, powers: &[G2Point]) -> G2Point {
        init();
        let n = self.coeffs.len();
        assert!(powers.len() >= n, "index out of bounds: the len is {} but the index is {}", powers.len(), powers.len());
        let p: Vec<ffi::zkt_g2_affine> = powers[..n].iter().map(|x| x.to_raw()).collect();
        let k = Fr::flatten(&self.coeffs);
        let mut out = G2Point::zero_raw();
        check(unsafe { ffi::zkt_g2_msm(p.as_ptr(), k.as_ptr(), n, &mut out) });
        G2Point::from_raw(&out)
    }
}

/// powers kept on the device with their window multiples (zkt_g1_bases): many evaluations against one CRS
pub struct G1Bases { h: *mut ffi::zkt_g1_bases, n: usize }
unsafe impl Send for G1Bases {}
impl G1Bases {
    pub fn upload(powers: &[G1Point]) -> Self {
        init();
        let p: Vec<ffi::zkt_g1_affine> = powers.iter().map(|x| x.to_raw()).collect();
        let mut h = std::ptr::null_mut();
        check(unsafe { ffi::zkt_g1_bases_upload(p.as_ptr(), p.len(), &mut h) });
        G1Bases { h, n: p.len() }
    }
    pub fn len(&self) -> usize { self.n }
    /// `dev_scalars`: n x 4 limbs already in HBM (a hipMalloc'ed buffer of the host application), on `stream`
    pub unsafe fn eval_dev(&self, dev_scalars: *const u64, stream: *mut std::os::raw::c_void) -> G1Point {
        let mut out = G1Point::zero_raw();
        check(ffi::zkt_g1_msm_dev(self.h, dev_scalars, self.n, stream, &mut out, std::ptr::null_mut()));
        G1Point::from_raw(&out)
    }
    pub fn raw(&self) -> *mut ffi::zkt_g1_bases { self.h }
}
impl Drop for G1Bases { fn drop(&mut self) { unsafe { ffi::zkt_g1_bases_free(self.h) } } }

pub struct G2Bases { h: *mut ffi::zkt_g2_bases, n: usize }
unsafe impl Send for G2Bases {}
impl G2Bases {
    pub fn upload(powers: &[G2Point]) -> Self {
        init();
        let p: Vec<ffi::zkt_g2_affine> = powers.iter().map(|x| x.to_raw()).collect();
        let mut h = std::ptr::null_mut();
        check(unsafe { ffi::zkt_g2_bases_upload(p.as_ptr(), p.len(), &mut h) });
        G2Bases { h, n: p.len() }
    }
    pub fn len(&self) -> usize { self.n }
    pub unsafe fn eval_dev(&self, dev_scalars: *const u64, stream: *mut std::os::raw::c_void) -> G2Point {
        let mut out = G2Point::zero_raw();
        check(ffi::zkt_g2_msm_dev(self.h, dev_scalars, self.n, stream, &mut out, std::ptr::null_mut()));
        G2Point::from_raw(&out)
    }
    pub fn raw(&self) -> *mut ffi::zkt_g2_bases { self.h }
}
impl Drop for G2Bases { fn drop(&mut self) { unsafe { ffi::zkt_g2_bases_free(self.h) } } }
