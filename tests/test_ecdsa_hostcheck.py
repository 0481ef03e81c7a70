"""The host build of csrc/sha256.h and csrc/ecdsa.h (libzkt_hostcheck.so: the same inline functions the kernels of zkt_ecdsa.hip run, compiled for the CPU)
against hashlib and the python-integer model of tests/ecdsa_model.py.  No GPU."""
import ctypes, hashlib, os, struct
import numpy as np
import pytest
from zkt_testlib import ROOT, SECP_N, SplitMix64, int_to_limbs, limbs_to_int
import ecdsa_model as M

SHA_LENGTHS = (0, 1, 3, 55, 56, 57, 63, 64, 65, 119, 120, 128, 1000)


@pytest.fixture(scope="module")
def H():
    so = os.path.join(ROOT, "zk-toolkit_amd", "libzkt_hostcheck.so")
    assert os.path.exists(so), "build first (__graft_entry__.build())"
    L = ctypes.CDLL(so)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.zkt_hostcheck_sha256.argtypes = [vp, sz, vp]
    L.zkt_hostcheck_sha256_compress.argtypes = [vp, vp]
    L.zkt_hostcheck_sha256_pad.argtypes = [vp, sz, sz, vp]
    L.zkt_hostcheck_ecdsa_verify.argtypes = [vp, vp, vp]
    L.zkt_hostcheck_ecdsa_sign.argtypes = [vp, vp, vp, vp]
    return L


def _sha(H, buf, start, length):
    out = np.zeros(32, dtype=np.uint8)
    H.zkt_hostcheck_sha256(buf.ctypes.data + start, length, out.ctypes.data)
    return out.tobytes()


def test_sha256_lengths_and_alignments(H):
    """every length on both sides of the 55/56 and 63/64 padding edges, at all four byte alignments of the message's start"""
    rng = np.random.Generator(np.random.PCG64(5))
    for length in SHA_LENGTHS:
        for align in range(4):
            buf = np.zeros(length + 16, dtype=np.uint8)
            base = (-buf.ctypes.data) % 4 + align                  # start address = align mod 4
            buf[base:base + length] = rng.integers(0, 256, size=length, dtype=np.uint8)
            assert _sha(H, buf, base, length) == hashlib.sha256(buf[base:base + length].tobytes()).digest(), (length, align)


def test_sha256_padding_is_pad_msg(H):
    """sha_common.rs:157-186: the message, 0x80, zeros up to 56 mod 64, the bit length in eight big-endian bytes"""
    for length in SHA_LENGTHS:
        msg = np.arange(length, dtype=np.uint64).astype(np.uint8) | np.uint8(1)
        plen = ctypes.c_size_t(0)
        zeros = (55 - length) % 64
        want = msg.tobytes() + b"\x80" + b"\x00" * zeros + struct.pack(">Q", 8 * length)
        got = bytes(H.zkt_hostcheck_sha256_pad(msg.ctypes.data, length, p, ctypes.byref(plen)) for p in range(len(want)))
        assert plen.value == len(want) and len(want) % 64 == 0 and got == want, length
        assert H.zkt_hostcheck_sha256_pad(msg.ctypes.data, length, len(want), None) == -1


def test_sha256_compression_of_the_abc_block(H):
    """one compression from the initial hash value over the padded block of "abc" is the digest (FIPS 180-4 example; sha256.rs:103-111)"""
    h = np.array([0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19], dtype=np.uint32)
    w = np.zeros(16, dtype=np.uint32); w[0] = 0x61626380; w[15] = 24
    H.zkt_hostcheck_sha256_compress(h.ctypes.data, w.ctypes.data)
    assert b"".join(struct.pack(">I", int(x)) for x in h) == hashlib.sha256(b"abc").digest()
    assert w[0] == 0x61626380 and w[15] == 24                       # the caller's block is not consumed


def test_verify_matches_the_model_on_the_full_case_list(H):
    cases = M.verify_cases()
    dig, sigs, pks = M.pack_cases(cases)
    kinds = set()
    for i, c in enumerate(cases):
        want = M.verify(c["z"], c["r"], c["s"], c["Q"])
        got = H.zkt_hostcheck_ecdsa_verify(dig[i].ctypes.data, sigs[i].ctypes.data, pks[i].ctypes.data)
        assert got == int(want), (i, c["kind"], got, want)
        kinds.add((c["kind"].split(" ")[0], want))
    # the constructed branches are in the list with the decisions the issue states
    for k in (("doubling", True), ("cancellation", False), ("wrap", True), ("valid", True), ("flip", False)):
        assert k in kinds, k


def test_sign_matches_the_model(H):
    rng = SplitMix64(11)
    cases = M.sign_cases() + [(M._b32(rng.below(1 << 256)), rng.below(1 << 256), rng.below(1 << 256)) for _ in range(12)]
    retries = 0
    for i, (zb, d, k) in enumerate(cases):
        z = np.frombuffer(zb, dtype=np.uint8).copy()
        da, ka = np.array(int_to_limbs(d, 4), dtype=np.uint64), np.array(int_to_limbs(k, 4), dtype=np.uint64)
        sig = np.full(8, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        retry = H.zkt_hostcheck_ecdsa_sign(z.ctypes.data, da.ctypes.data, ka.ctypes.data, sig.ctypes.data)
        want = M.sign(zb, d, k)
        if want == M.RETRY:
            retries += 1
            assert retry == 1 and not sig.any(), i
        else:
            assert retry == 0 and (limbs_to_int(sig[:4]), limbs_to_int(sig[4:])) == want, i
            assert M.verify(zb, want[0], want[1], M.gen_pub_key(d)) == (d % SECP_N != 0)      # d = 0 mod n signs, but its key is the point at infinity (:94)
    assert retries == 4                                               # k = 0, k = n, and the two s == 0 constructions
