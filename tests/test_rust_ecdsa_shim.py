"""bindings/rust/src/ecdsa.rs is shipped as source (no rustc here, as tests/test_rust_shim.py explains): the reference's names and signatures
(ecdsa.rs:16-35, :37, :88; sha256.rs:33-34, :76), the retry loop of sign, and the two module paths are checked on the text."""
import os, re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RS = os.path.join(ROOT, "bindings", "rust", "src")


def _norm(t):
    return re.sub(r"\s+", " ", re.sub(r"//.*", "", t))


def test_reference_signatures_verbatim():
    src = _norm(open(os.path.join(RS, "ecdsa.rs")).read())
    for needle in ("pub struct Signature { pub r: PrimeFieldElem, pub s: PrimeFieldElem }",                     # ecdsa.rs:17-20
                   "pub struct Ecdsa { pub hasher: Sha256 }",                                                   # :22-24
                   "pub fn new(hasher: &Sha256) -> Self",                                                       # :27
                   "pub fn gen_pub_key(&self, priv_key: &PrimeFieldElem) -> AffinePoint",                       # :33
                   "pub fn sign(&self, priv_key: &PrimeFieldElem, message: &[u8]) -> Result<Signature, String>",  # :37
                   "pub fn verify(&self, sig: &Signature, pub_key: &AffinePoint, message: &[u8]) -> bool",      # :88
                   "pub struct Sha256();",                                                                      # sha256.rs:34
                   "pub fn get_digest(&self, msg: &[u8]) -> [u8; 32]"):                                         # sha256.rs:76
        assert needle in src, needle
    # the elements are the runtime-order ones, whose integer can be n or more: verification must see r and s as given
    assert "use crate::building_block::field::prime_field_elem::PrimeFieldElem;" in src
    assert "to_limbs(&sig.r.e, 4)" in src and "to_limbs(&sig.s.e, 4)" in src


def test_sign_draws_k_and_loops_on_retry():
    src = _norm(open(os.path.join(RS, "ecdsa.rs")).read())
    body = src[src.index("pub fn sign(&self"):src.index("pub fn verify(&self")]
    order = [body.index(k) for k in ("loop {", "let k = f_n.rand_elem(true);", "ffi::zkt_ecdsa_sign_batch(", "if retry != 0 { continue; }", "return Ok(Signature {")]
    assert order == sorted(order)
    assert 'panic!("Private key needs to be an element of curve group")' in body                               # ecdsa.rs:40-42


def test_every_entry_point_is_bound():
    src = open(os.path.join(RS, "ecdsa.rs")).read()
    for fn in ("zkt_sha256_batch", "zkt_ecdsa_public_keys_batch", "zkt_ecdsa_sign_batch", "zkt_ecdsa_verify_batch"):
        assert "ffi::" + fn + "(" in src, fn
    ffi = open(os.path.join(RS, "ffi.rs")).read()
    assert re.search(r"pub struct zkt_ecdsa_sig \{\s*pub r: \[u64; 4\],\s*pub s: \[u64; 4\],\s*\}", ffi)
    for fn in ("zkt_ecdsa_sign_digest_batch", "zkt_ecdsa_verify_digest_batch", "zkt_ecdsa_verify_digest_batch_dev"):
        assert "pub fn " + fn + "(" in ffi, fn


def test_reference_module_paths():
    src = open(os.path.join(RS, "reference_paths.rs")).read()
    lib = open(os.path.join(RS, "lib.rs")).read()
    assert "pub mod ecdsa;" in lib
    def has_path(path, items):
        pos = 0
        for seg in path.split("::"):
            pos = src.find("pub mod %s" % seg, pos)
            assert pos >= 0, f"{path}: module {seg} missing"
        tail = src[pos:pos + 200]
        for item in items:
            assert re.search(r"pub use crate::ecdsa::[^;]*\b%s\b" % item, tail), f"{path}::{item} not exported"
    has_path("building_block::curves::secp256k1::ecdsa", ("Ecdsa", "Signature"))
    has_path("building_block::hasher::sha256", ("Sha256",))
    body = open(os.path.join(RS, "ecdsa.rs")).read()
    for item in ("Ecdsa", "Signature", "Sha256"):
        assert re.search(r"pub struct %s\b" % item, body)
