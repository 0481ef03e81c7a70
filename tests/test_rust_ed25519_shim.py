"""bindings/rust/src/ed25519.rs is shipped as source (no rustc here, as tests/test_rust_shim.py explains): the reference's names and signatures
(ed25519_sha512.rs:21-35, :115, :127, :160; sha512.rs:37-38, :92), the bound entry points and the two module paths are checked on the text."""
import os, re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RS = os.path.join(ROOT, "bindings", "rust", "src")
RUST_KEYWORDS = {"pub", "fn", "mod", "use", "type", "match", "ref", "in", "move", "impl", "self", "where", "loop", "as", "box", "dyn", "priv"}


def _norm(t):
    return re.sub(r"\s+", " ", re.sub(r"//.*", "", t))


def test_reference_signatures_verbatim():
    src = _norm(open(os.path.join(RS, "ed25519.rs")).read())
    for needle in ("pub struct KeyPair { pub prv_key: [u8; 32], pub pub_key: [u8; 32], }",                      # ed25519_sha512.rs:22-25
                   "pub struct Ed25519Sha512 { H: Sha512, }",                                                    # :28-30
                   "pub fn new() -> Self",                                                                       # :33
                   "pub fn gen_pub_key(&self, prv_key: &[u8; 32]) -> [u8; 32]",                                  # :115
                   "pub fn sign(&self, msg: &[u8], prv_key: &[u8; 32]) -> [u8; 64]",                             # :127
                   "pub fn verify(&self, sig: &[u8;64], pub_key: &[u8; 32], msg: &[u8]) -> bool",                # :160
                   "pub struct Sha512();",                                                                       # sha512.rs:38
                   "pub fn get_digest(&self, msg: &[u8]) -> [u8; 64]"):                                          # sha512.rs:92
        assert needle in src, needle


def test_every_entry_point_is_bound():
    src = open(os.path.join(RS, "ed25519.rs")).read()
    fns = ("zkt_sha512_batch", "zkt_ed25519_decode_batch", "zkt_ed25519_public_keys_batch", "zkt_ed25519_sign_batch", "zkt_ed25519_verify_batch")
    for fn in fns:
        assert "ffi::" + fn + "(" in src, fn
    ffi = open(os.path.join(RS, "ffi.rs")).read()
    for fn in fns + ("zkt_ed25519_verify_batch_dev",):
        m = re.search(r"pub fn %s\(([^)]*)\)" % fn, ffi)
        assert m, fn
        names = [a.split(":")[0].strip() for a in m.group(1).split(",")]
        assert not set(names) & RUST_KEYWORDS, (fn, names)          # a C parameter called `pub` would not compile
    for needle in ("pub fn gen_pub_keys_batch(", "pub fn sign_batch(", "pub fn verify_batch(", "pub fn get_digests(", "pub fn decode_points_batch("):
        assert needle in src, needle


def test_reference_module_paths():
    src = open(os.path.join(RS, "reference_paths.rs")).read()
    lib = open(os.path.join(RS, "lib.rs")).read()
    assert "pub mod ed25519;" in lib
    def has_path(path, items):
        pos = 0
        for seg in path.split("::"):
            pos = src.find("pub mod %s" % seg, pos)
            assert pos >= 0, f"{path}: module {seg} missing"
        tail = src[pos:pos + 200]
        for item in items:
            assert re.search(r"pub use crate::ed25519::[^;]*\b%s\b" % item, tail), f"{path}::{item} not exported"
    has_path("building_block::curves::curve25519::ed25519_sha512", ("Ed25519Sha512", "KeyPair"))
    has_path("building_block::hasher::sha512", ("Sha512",))
    body = open(os.path.join(RS, "ed25519.rs")).read()
    for item in ("Ed25519Sha512", "KeyPair", "Sha512"):
        assert re.search(r"pub struct %s\b" % item, body)
