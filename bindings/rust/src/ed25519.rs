//! Ed25519 over SHA-512 — building_block/curves/curve25519/ed25519_sha512.rs:21-186, building_block/hasher/sha512.rs:37-102.
//! The reference's names and signatures over the batched entry points: one key or one signature is a batch of one; `gen_pub_keys_batch` / `sign_batch` /
//! `verify_batch` / `get_digests` are what a hot loop should call (one launch, one lane per element).  Everything is bytes, as in the reference.
use crate::ffi;
use crate::{check, init};

/// sha512.rs:37-38
#[derive(Clone)]
pub struct Sha512();

fn offsets(msgs: &[&[u8]]) -> (Vec<u8>, Vec<u64>) {
    let mut flat = Vec::new();
    let mut off = vec![0u64];
    for m in msgs { flat.extend_from_slice(m); off.push(flat.len() as u64); }
    (flat, off)
}

impl Sha512 {
    /// Hasher::get_digest (sha512.rs:91-97)
    pub fn get_digest(&self, msg: &[u8]) -> [u8; 64] { self.get_digests(&[msg]).remove(0) }
    /// sha512.rs:99-101
    pub fn get_block_size(&self) -> usize { 128 }
    /// n messages, one launch, one lane per message
    pub fn get_digests(&self, msgs: &[&[u8]]) -> Vec<[u8; 64]> {
        init();
        let (flat, off) = offsets(msgs);
        let mut out = vec![[0u8; 64]; msgs.len()];
        check(unsafe { ffi::zkt_sha512_batch(flat.as_ptr(), off.as_ptr(), msgs.len(), out.as_mut_ptr() as *mut u8) });
        out
    }
}

/// ed25519_sha512.rs:21-25
#[derive(Debug)]
pub struct KeyPair {
    pub prv_key: [u8; 32],
    pub pub_key: [u8; 32],
}

/// ed25519_sha512.rs:27-30
#[derive(Clone)]
#[allow(non_snake_case)]
pub struct Ed25519Sha512 {
    H: Sha512,
}

impl Ed25519Sha512 {
    pub fn new() -> Self { init(); Ed25519Sha512 { H: Sha512() } } // :33-35

    /// :115-125
    pub fn gen_pub_key(&self, prv_key: &[u8; 32]) -> [u8; 32] { self.gen_pub_keys_batch(&[*prv_key]).remove(0) }

    /// :127-158 (deterministic)
    pub fn sign(&self, msg: &[u8], prv_key: &[u8; 32]) -> [u8; 64] { self.sign_batch(&[msg], &[*prv_key]).remove(0) }

    /// :160-186
    pub fn verify(&self, sig: &[u8;64], pub_key: &[u8; 32], msg: &[u8]) -> bool { self.verify_batch(&[*sig], &[*pub_key], &[msg])[0] }

    /// decode_point (:85-98) for n encodings: (x, y) as canonical little-endian limbs and whether the point is on the curve
    pub fn decode_points_batch(&self, enc: &[[u8; 32]]) -> Vec<([u64; 4], [u64; 4], bool)> {
        let mut xy = vec![[0u64; 8]; enc.len()];
        let mut on = vec![0u32; enc.len()];
        check(unsafe { ffi::zkt_ed25519_decode_batch(enc.as_ptr() as *const u8, enc.len(), xy.as_mut_ptr() as *mut u64, on.as_mut_ptr()) });
        xy.iter().zip(&on).map(|(p, f)| ([p[0], p[1], p[2], p[3]], [p[4], p[5], p[6], p[7]], *f == 1)).collect()
    }

    /// n private keys, one launch
    pub fn gen_pub_keys_batch(&self, prv_keys: &[[u8; 32]]) -> Vec<[u8; 32]> {
        let mut out = vec![[0u8; 32]; prv_keys.len()];
        check(unsafe { ffi::zkt_ed25519_public_keys_batch(prv_keys.as_ptr() as *const u8, prv_keys.len(), out.as_mut_ptr() as *mut u8) });
        out
    }

    /// n key pairs, one launch
    pub fn gen_key_pairs_batch(&self, prv_keys: &[[u8; 32]]) -> Vec<KeyPair> {
        self.gen_pub_keys_batch(prv_keys).iter().zip(prv_keys).map(|(p, s)| KeyPair { prv_key: *s, pub_key: *p }).collect()
    }

    /// n (message, private key) pairs, one launch, one lane per signature
    pub fn sign_batch(&self, msgs: &[&[u8]], prv_keys: &[[u8; 32]]) -> Vec<[u8; 64]> {
        assert!(msgs.len() == prv_keys.len());
        let (flat, off) = offsets(msgs);
        let mut out = vec![[0u8; 64]; msgs.len()];
        check(unsafe { ffi::zkt_ed25519_sign_batch(flat.as_ptr(), off.as_ptr(), prv_keys.as_ptr() as *const u8, msgs.len(), out.as_mut_ptr() as *mut u8) });
        out
    }

    /// n signatures, one launch, one lane per signature
    pub fn verify_batch(&self, sigs: &[[u8; 64]], pub_keys: &[[u8; 32]], msgs: &[&[u8]]) -> Vec<bool> {
        assert!(sigs.len() == msgs.len() && pub_keys.len() == msgs.len());
        let (flat, off) = offsets(msgs);
        let mut ok = vec![0u32; msgs.len()];
        check(unsafe { ffi::zkt_ed25519_verify_batch(flat.as_ptr(), off.as_ptr(), sigs.as_ptr() as *const u8, pub_keys.as_ptr() as *const u8, msgs.len(), ok.as_mut_ptr()) });
        ok.iter().map(|v| *v == 1).collect()
    }

    /// the hasher this instance was made with (ed25519_sha512.rs:28)
    pub fn hasher(&self) -> &Sha512 { &self.H }
}
