"""The host build of csrc/sha512.h, csrc/fe25519.h and csrc/ed25519.h (libzkt_hostcheck.so: the same inline functions the kernels of zkt_ed25519.hip run,
compiled for the CPU) against hashlib, python integers and the model of tests/ed25519_model.py.  No GPU."""
import ctypes, hashlib, os
import numpy as np
import pytest
from zkt_testlib import ROOT
import ed25519_model as M

Q, L = M.Q, M.L
SHA_LENGTHS = (0, 1, 3, 111, 112, 113, 127, 128, 129, 239, 240, 256, 1000)


@pytest.fixture(scope="module")
def H():
    so = os.path.join(ROOT, "zk-toolkit_amd", "libzkt_hostcheck.so")
    assert os.path.exists(so), "build first (__graft_entry__.build())"
    lib = ctypes.CDLL(so)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    lib.zkt_hostcheck_sha512.argtypes = [vp, sz, vp, sz, vp]
    lib.zkt_hostcheck_sha512_compress.argtypes = [vp, vp]
    lib.zkt_hostcheck_sha512_pad.argtypes = [vp, sz, sz, vp]
    lib.zkt_hostcheck_fe25519_mul.argtypes = [vp, vp, vp]
    lib.zkt_hostcheck_fe25519_sqr.argtypes = [vp, vp]
    lib.zkt_hostcheck_fe25519_inv.argtypes = [vp, vp]
    lib.zkt_hostcheck_fe25519_lin.argtypes = [ci, vp, vp, vp]
    lib.zkt_hostcheck_fe25519_sqrt_ratio.argtypes = [vp, vp, vp]
    lib.zkt_hostcheck_sc25519_reduce512.argtypes = [vp, vp]
    lib.zkt_hostcheck_sc25519_muladd.argtypes = [vp, vp, vp, vp]
    lib.zkt_hostcheck_ed25519_decode.argtypes = [vp, vp]
    lib.zkt_hostcheck_ed25519_pub_from_scalar.argtypes = [vp, vp]
    lib.zkt_hostcheck_ed25519_public_key.argtypes = [vp, vp]
    lib.zkt_hostcheck_ed25519_sign.argtypes = [vp, sz, vp, vp]
    lib.zkt_hostcheck_ed25519_verify.argtypes = [vp, sz, vp, vp, ci]
    return lib


def _w(v, n=8): return np.frombuffer(int(v).to_bytes(4 * n, "little"), dtype=np.uint32).copy()
def _i(a): return int.from_bytes(a.tobytes(), "little")
def _b(b): return np.frombuffer(bytes(b) or b"\0", dtype=np.uint8).copy()
def _c(fn, *args):
    """call with numpy arrays passed by address; the arrays stay referenced until the call returns"""
    return fn(*[a.ctypes.data if isinstance(a, np.ndarray) else a for a in args])


# ---- SHA-512 -----------------------------------------------------------------------------------------------------------------------------------------
def _sha(H, buf, start, length, prefix=b""):
    out = np.zeros(64, dtype=np.uint8)
    pre = _b(prefix)
    assert H.zkt_hostcheck_sha512(pre.ctypes.data, len(prefix), buf.ctypes.data + start, length, out.ctypes.data) == 0
    return out.tobytes()


def test_sha512_every_length_at_every_alignment(H):
    rng = np.random.Generator(np.random.PCG64(512))
    buf = rng.integers(0, 256, size=1100, dtype=np.uint8)
    base = (-buf.ctypes.data) % 8                                 # start offsets are relative to an 8-byte boundary
    for length in SHA_LENGTHS:
        for a in range(8):
            s = base + a
            assert _sha(H, buf, s, length) == hashlib.sha512(buf[s:s + length].tobytes()).digest(), (length, a)


def test_sha512_register_prefix_forms(H):
    """prefix ‖ msg with the 32- or 64-byte prefix in registers, at the block edges of both strings and every alignment of the message"""
    rng = np.random.Generator(np.random.PCG64(513))
    buf = rng.integers(0, 256, size=1200, dtype=np.uint8)
    base = (-buf.ctypes.data) % 8
    for plen in (32, 64):
        prefix = rng.integers(0, 256, size=plen, dtype=np.uint8).tobytes()
        for length in M.MSG_LENGTHS + (111, 112, 113, 128, 200):
            for a in (0, 1, 3, 4, 7):
                s = base + a
                assert _sha(H, buf, s, length, prefix) == hashlib.sha512(prefix + buf[s:s + length].tobytes()).digest(), (plen, length, a)


def _pad_msg(msg):
    """pad_msg of sha_common.rs:157-186 for BLOCK_SIZE 128, LENGTH_PART_LEN 16"""
    v = bytearray(msg) + b"\x80"
    last = len(v) % 128
    v += bytes(112 - last if last <= 112 else 128 - last + 112)
    return bytes(v) + (len(msg) * 8).to_bytes(16, "big")


def test_sha512_padding_is_pad_msg(H):
    for length in SHA_LENGTHS + (110, 114, 238, 241):
        msg = np.full(max(length, 1), 0x81, dtype=np.uint8)
        want = _pad_msg(msg[:length].tobytes())
        plen = ctypes.c_size_t(0)
        got = bytes(H.zkt_hostcheck_sha512_pad(msg.ctypes.data, length, p, ctypes.byref(plen)) for p in range(len(want)))
        assert plen.value == len(want) and got == want, length
        assert H.zkt_hostcheck_sha512_pad(msg.ctypes.data, length, len(want), None) == -1


def test_sha512_one_compression_of_abc(H):
    h = np.array([0x6a09e667f3bcc908, 0xbb67ae8584caa73b, 0x3c6ef372fe94f82b, 0xa54ff53a5f1d36f1, 0x510e527fade682d1, 0x9b05688c2b3e6c1f, 0x1f83d9abfb41bd6b,
                  0x5be0cd19137e2179], dtype=np.uint64)
    w = np.frombuffer(_pad_msg(b"abc"), dtype=">u8").astype(np.uint64)
    H.zkt_hostcheck_sha512_compress(h.ctypes.data, w.ctypes.data)
    assert b"".join(int(x).to_bytes(8, "big") for x in h) == hashlib.sha512(b"abc").digest()


# ---- the field -----------------------------------------------------------------------------------------------------------------------------------------
def _field_values():
    rng = M._Rng(25519)
    # 2^256 - 1 is every limb 0xffffffff before the canonical reduction: the form admits every 256-bit value
    return [0, 1, 2, Q - 1, 2 ** 255 - 20, Q, Q + 1, 2 * Q, 2 * Q + 37, 2 ** 256 - 1, 2 ** 256 - 38, 2 ** 255, 19, 38] + [rng.below(2 ** 256) for _ in range(64)]


def test_fe25519_mul_sqr_and_linear_ops(H):
    vals = _field_values()
    o = np.zeros(8, np.uint32)
    for i, a in enumerate(vals):
        b = vals[(i * 7 + 3) % len(vals)]
        for bb in (b, a, 2 ** 256 - 1):
            _c(H.zkt_hostcheck_fe25519_mul, _w(a), _w(bb), o); assert _i(o) == a * bb % Q, (a, bb)
            for op, want in ((0, a + bb), (1, a - bb), (2, -a)):
                _c(H.zkt_hostcheck_fe25519_lin, op, _w(a), _w(bb), o); assert _i(o) == want % Q, (op, a, bb)
        _c(H.zkt_hostcheck_fe25519_sqr, _w(a), o); assert _i(o) == a * a % Q, a


def test_fe25519_inverse(H):
    o = np.zeros(8, np.uint32)
    for a in _field_values():
        _c(H.zkt_hostcheck_fe25519_inv, _w(a), o)
        assert _i(o) == pow(a % Q, Q - 2, Q), a               # 0 for 0


def test_fe25519_sqrt_ratio_is_the_reference_root(H):
    """x = (u/v)^((q+3)/8), times I when its square is not u/v, nothing further (affine_point.rs:92-99)"""
    vals = [v for v in _field_values()]
    x = np.zeros(8, np.uint32)
    flags = []
    for i, u in enumerate(vals):
        v = vals[(i * 5 + 1) % len(vals)]
        if v % Q == 0: v = 7
        xx = u * pow(v, Q - 2, Q) % Q
        want = pow(xx, (Q + 3) // 8, Q)
        if want * want % Q != xx: want = want * M.I % Q
        ok = _c(H.zkt_hostcheck_fe25519_sqrt_ratio, _w(u), _w(v), x)
        assert _i(x) == want and ok == int(want * want % Q == xx), (u, v)
        flags.append(ok)
    assert 10 < sum(flags) < len(flags) - 10


# ---- integers mod l --------------------------------------------------------------------------------------------------------------------------------------
def test_sc25519_reduce512(H):
    rng = M._Rng(252)
    r = np.zeros(8, np.uint32)
    edges = [0, L - 1, L, L + 1, 2 ** 252, 2 ** 512 - 1, 2 ** 252 - 1, 2 * L, 2 ** 256 - 1, 2 ** 256, L << 259, (L << 259) - 1, 2 ** 511]
    for x in edges + [rng.below(2 ** 512) for _ in range(64)]:
        _c(H.zkt_hostcheck_sc25519_reduce512, _w(x, 16), r)
        assert _i(r) == x % L, hex(x)


def test_sc25519_muladd(H):
    rng = M._Rng(253)
    r = np.zeros(8, np.uint32)
    edges = [0, 1, L - 1, L, L + 1, 2 ** 252, 2 ** 256 - 1, 2 ** 255 - 8]
    trip = [(a, b, c) for a in edges for b in edges for c in (0, L - 1, 2 ** 256 - 1)] + [tuple(rng.below(2 ** 256) for _ in range(3)) for _ in range(64)]
    for a, b, c in trip:
        _c(H.zkt_hostcheck_sc25519_muladd, _w(a), _w(b), _w(c), r)
        assert _i(r) == (a * b + c) % L, (a, b, c)


# ---- decode, keys, signatures ------------------------------------------------------------------------------------------------------------------------------
def test_decode_every_case_x_y_and_flag(H):
    xy = np.zeros(16, np.uint32)
    flags = []
    for enc in M.decode_cases():
        on = _c(H.zkt_hostcheck_ed25519_decode, _b(enc), xy)
        x, y, want = M.decode_want(enc)
        assert (_i(xy[:8]), _i(xy[8:]), on) == (x, y, int(want)), enc.hex()
        flags.append(on)
    assert min(sum(flags), len(flags) - sum(flags)) >= 10
    # the named edges: y = q + 1 is (0, 1); y = q is an order-4 point (+-I, 0); y = 1 with the sign bit set stays x = 0
    assert M.decode_want((Q + 1).to_bytes(32, "little")) == (0, 1, True)
    assert M.decode_want(Q.to_bytes(32, "little"))[1:] == (0, True) and M.decode_want(Q.to_bytes(32, "little"))[0] in (M.I, Q - M.I)
    assert M.decode_want((1 | 1 << 255).to_bytes(32, "little")) == (0, 1, True)


def test_pub_from_scalar_reduces_s_mod_q(H):
    """base_field().elem(&s) (ed25519_sha512.rs:121): s = 2^255 - 8 and 2^255 - 16 multiply B by 11 and 3"""
    pub = np.zeros(32, np.uint8)
    rng = M._Rng(31)
    pruned = [M.gen_s(rng.bytes(32)) for _ in range(8)]
    for s in [2 ** 255 - 8, 2 ** 255 - 16] + pruned:
        _c(H.zkt_hostcheck_ed25519_pub_from_scalar, _b(s.to_bytes(32, "little")), pub)
        assert pub.tobytes() == M.pub_from_scalar(s), hex(s)
    assert M.pub_from_scalar(2 ** 255 - 8) == M.encode_point(M.fast_mul(M.B, 11)) and M.pub_from_scalar(2 ** 255 - 16) == M.encode_point(M.fast_mul(M.B, 3))
    assert M.pub_from_scalar(2 ** 255 - 8) != M.encode_point(M.fast_mul(M.B, (2 ** 255 - 8) % L))


def test_public_keys_and_signatures_match_the_model(H):
    pub, sig = np.zeros(32, np.uint8), np.zeros(64, np.uint8)
    for prv, msg in M.sign_cases():
        _c(H.zkt_hostcheck_ed25519_public_key, _b(prv), pub)
        assert pub.tobytes() == M.gen_pub_key(prv)
        m = _b(msg)
        _c(H.zkt_hostcheck_ed25519_sign, m, len(msg), _b(prv), sig)
        assert sig.tobytes() == M.sign(msg, prv), (prv.hex(), len(msg))
    for v in M.vectors():
        assert M.sign(v["msg_hex"], v["prv"]) == v["sig"] and M.gen_pub_key(v["prv"]) == v["pub"]


@pytest.mark.parametrize("stride", [1, 64])
def test_verify_matches_the_model_on_the_full_case_list(H, stride):
    cases = M.verify_cases()
    for i, c in enumerate(cases):
        m = _b(c["msg"])
        got = _c(H.zkt_hostcheck_ed25519_verify, m, len(c["msg"]), _b(c["sig"]), _b(c["pub"]), stride)
        assert got == int(c["want"]), (i, c["kind"])


def test_under_address_and_undefined_sanitizers(tmp_path):
    """tests/c/ed25519_check.cpp (its own main: sign, verify and hash at every alignment on exact-size heap blocks) built for the host with the address and
    undefined-behaviour sanitizers and run as a program of its own; nothing is loaded into python"""
    import subprocess
    exe = tmp_path / "ed25519_check"
    subprocess.check_call(["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-option-ignored",
                           "-Wno-unused-value", "-Wno-unused-result", "-I", os.path.join(ROOT, "zk-toolkit_amd", "csrc"), os.path.join(ROOT, "tests", "c", "ed25519_check.cpp"), "-o", str(exe)], timeout=900)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "ed25519 ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
