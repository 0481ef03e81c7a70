//! secp256k1 ECDSA and SHA-256 — building_block/curves/secp256k1/ecdsa.rs:16-135, building_block/hasher/sha256.rs:34-86.
//! The reference's names and signatures over the batched entry points: one signature is a batch of one; `sign_batch` / `verify_batch` / `get_digests`
//! are what a hot loop should call (one launch, one lane per signature).
use crate::building_block::field::prime_field::PrimeField;
use crate::building_block::field::prime_field_elem::PrimeFieldElem;
use crate::ffi;
use crate::field::{to_limbs, from_limbs, FieldSpec, SecpN};
use crate::points::{AffinePoint, SecpPoint};
use crate::{check, init};
use std::sync::Arc;

/// sha256.rs:33-34
#[derive(Clone)]
pub struct Sha256();

fn offsets(msgs: &[&[u8]]) -> (Vec<u8>, Vec<u64>) {
    let mut flat = Vec::new();
    let mut off = vec![0u64];
    for m in msgs { flat.extend_from_slice(m); off.push(flat.len() as u64); }
    (flat, off)
}

impl Sha256 {
    /// Hasher::get_digest (sha256.rs:75-81)
    pub fn get_digest(&self, msg: &[u8]) -> [u8; 32] { self.get_digests(&[msg]).remove(0) }
    /// sha256.rs:83-85
    pub fn get_block_size(&self) -> usize { 64 }
    /// n messages, one launch, one lane per message
    pub fn get_digests(&self, msgs: &[&[u8]]) -> Vec<[u8; 32]> {
        init();
        let (flat, off) = offsets(msgs);
        let mut out = vec![[0u8; 32]; msgs.len()];
        check(unsafe { ffi::zkt_sha256_batch(flat.as_ptr(), off.as_ptr(), msgs.len(), out.as_mut_ptr() as *mut u8) });
        out
    }
}

/// ecdsa.rs:16-20.  `r` and `s` are the reference's runtime-order elements: verification reads their integers `e` as given and compares them with n
/// (:105-112), so a value that is not below n — the reference's own tests build r = n as an element of the base field, :211-214 — stays what it is.
#[derive(Debug, Clone)]
pub struct Signature { pub r: PrimeFieldElem, pub s: PrimeFieldElem }

/// ecdsa.rs:22-24
pub struct Ecdsa { pub hasher: Sha256 }

fn curve_group() -> Arc<PrimeField> { Arc::new(PrimeField::new(&SecpN::order())) } // affine_point.rs:34-38

fn raw_sig(sig: &Signature) -> ffi::zkt_ecdsa_sig {
    let (r, s) = (to_limbs(&sig.r.e, 4), to_limbs(&sig.s.e, 4));
    ffi::zkt_ecdsa_sig { r: [r[0], r[1], r[2], r[3]], s: [s[0], s[1], s[2], s[3]] }
}

impl Ecdsa {
    pub fn new(hasher: &Sha256) -> Self { init(); Ecdsa { hasher: hasher.clone() } } // :27-31

    /// AffinePoint::g() * priv_key (:33-35)
    pub fn gen_pub_key(&self, priv_key: &PrimeFieldElem) -> AffinePoint {
        let k = to_limbs(&priv_key.e, 4);
        let mut out = SecpPoint::zero_raw();
        check(unsafe { ffi::zkt_ecdsa_public_keys_batch(k.as_ptr(), 1, &mut out) });
        SecpPoint::from_raw(&out)
    }

    /// :37-85 — draws k where the reference does (:51) and loops while the library reports `retry` (k G at infinity :61, r == 0 :67, s == 0 :77)
    pub fn sign(&self, priv_key: &PrimeFieldElem, message: &[u8]) -> Result<Signature, String> {
        let f_n = curve_group();
        if priv_key.f.order_ref() != f_n.order_ref() { panic!("Private key needs to be an element of curve group"); } // :40-42
        let d = to_limbs(&priv_key.e, 4);
        let off = [0u64, message.len() as u64];
        loop {
            let k = f_n.rand_elem(true); // :51
            let kl = to_limbs(&k.e, 4);
            let mut sig = ffi::zkt_ecdsa_sig { r: [0; 4], s: [0; 4] };
            let mut retry = 0u32;
            check(unsafe { ffi::zkt_ecdsa_sign_batch(message.as_ptr(), off.as_ptr(), d.as_ptr(), kl.as_ptr(), 1, &mut sig, &mut retry) });
            if retry != 0 { continue; } // :61, :67, :77
            return Ok(Signature { r: f_n.elem(&from_limbs(&sig.r)), s: f_n.elem(&from_limbs(&sig.s)) }); // :81
        }
    }

    /// :88-135
    pub fn verify(&self, sig: &Signature, pub_key: &AffinePoint, message: &[u8]) -> bool {
        self.verify_batch(&[sig.clone()], &[pub_key.clone()], &[message])[0]
    }

    /// n (private key, nonce, message) triples, one launch; `None` where the reference would draw another nonce
    pub fn sign_batch(&self, priv_keys: &[PrimeFieldElem], nonces: &[PrimeFieldElem], messages: &[&[u8]]) -> Vec<Option<Signature>> {
        assert!(priv_keys.len() == messages.len() && nonces.len() == messages.len());
        let f_n = curve_group();
        let n = messages.len();
        let (flat, off) = offsets(messages);
        let d: Vec<u64> = priv_keys.iter().flat_map(|x| to_limbs(&x.e, 4)).collect();
        let k: Vec<u64> = nonces.iter().flat_map(|x| to_limbs(&x.e, 4)).collect();
        let mut sigs = vec![ffi::zkt_ecdsa_sig { r: [0; 4], s: [0; 4] }; n];
        let mut retry = vec![0u32; n];
        check(unsafe { ffi::zkt_ecdsa_sign_batch(flat.as_ptr(), off.as_ptr(), d.as_ptr(), k.as_ptr(), n, sigs.as_mut_ptr(), retry.as_mut_ptr()) });
        sigs.iter().zip(&retry).map(|(s, r)| if *r != 0 { None } else { Some(Signature { r: f_n.elem(&from_limbs(&s.r)), s: f_n.elem(&from_limbs(&s.s)) }) }).collect()
    }

    /// n signatures, one launch, one lane per signature
    pub fn verify_batch(&self, sigs: &[Signature], pub_keys: &[AffinePoint], messages: &[&[u8]]) -> Vec<bool> {
        assert!(sigs.len() == messages.len() && pub_keys.len() == messages.len());
        let (flat, off) = offsets(messages);
        let s: Vec<ffi::zkt_ecdsa_sig> = sigs.iter().map(raw_sig).collect();
        let p: Vec<ffi::zkt_secp_affine> = pub_keys.iter().map(|x| x.to_raw()).collect();
        let mut ok = vec![0u32; messages.len()];
        check(unsafe { ffi::zkt_ecdsa_verify_batch(flat.as_ptr(), off.as_ptr(), s.as_ptr(), p.as_ptr(), messages.len(), ok.as_mut_ptr()) });
        ok.iter().map(|v| *v == 1).collect()
    }
}
