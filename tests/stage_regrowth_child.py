"""Child process of tests/test_gpu_api_status.py::test_arena_regrowth_between_layouts (TEST INFRASTRUCTURE; ctypes only, so the staging arena starts at zero bytes).

Three host-pointer calls with different slot lists share the arena: zkt_fr_mul_batch (3 slots), zkt_sha512_batch (messages, offsets, digests) and
zkt_ed25519_verify_batch (5 slots).  Every ascending step asks for more than the arena holds after the step before (1.25 x that request + 1 MiB), so the arena is
freed and allocated again between calls and every pointer of the next call comes from the new block; then the sizes go back down to one element.

  step            request (bytes: the slot sizes rounded up to 256 each)                       arena after it (request + request/4 + 2^20)
  fr      1       3 x 256                                                    =        768        1 049 536
  fr      20 000  3 x 640 000                                                =  1 920 000        3 448 576
  sha512  30 000  1 920 000 + 240 128 (30 001 offsets) + 1 920 000           =  4 080 128        6 148 736
  fr     200 000  3 x 6 400 000                                              = 19 200 000       25 048 576
  sha512 200 000  12 800 000 + 1 600 256 (200 001 offsets) + 12 800 000      = 27 200 256       35 048 896
The Ed25519 batches (at most 256 signatures of 64-byte messages: 16 384 + 2 304 + 16 384 + 8 192 + 1 024 = 44 288 bytes) never grow it: they run inside
whatever block the step before left.  Exit status 0 and a last line "ok", or an AssertionError."""
import ctypes, hashlib, os, sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ed25519_model as M

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
ZKT_OK, ZKT_ERR_SHAPE, ZKT_ERR_DEVICE = 0, 3, 4
vp, sz = ctypes.c_void_p, ctypes.c_size_t
L = ctypes.CDLL(os.environ.get("ZKT_LIB_PATH", os.path.join(os.path.dirname(HERE), "zk-toolkit_amd", "libzkt_hip.so")))      # the override is the package's own
L.zkt_fr_mul_batch.argtypes = [vp, vp, vp, sz]
L.zkt_sha512_batch.argtypes = [vp, vp, sz, vp]
L.zkt_ed25519_verify_batch.argtypes = [vp, vp, vp, vp, sz, vp]
L.zkt_ecdsa_sign_digest_batch.argtypes = [vp, vp, vp, sz, vp, vp]
L.zkt_ecdsa_verify_digest_batch.argtypes = [vp, vp, vp, sz, vp]
p_ = lambda a: a.ctypes.data
rng = np.random.Generator(np.random.PCG64(2024))


def fr_ints(a):
    raw = a.tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(a))]


def fr_mul(n):
    a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64); b = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(2); b[:, 3] >>= np.uint64(2)                      # below 2^254 < r: canonical
    out = np.full((n, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    assert L.zkt_fr_mul_batch(p_(a), p_(b), p_(out), n) == ZKT_OK
    assert fr_ints(out) == [x * y % R for x, y in zip(fr_ints(a), fr_ints(b))], ("fr_mul", n)


def sha512(n):
    buf = rng.integers(0, 256, size=n * 64, dtype=np.uint8); off = np.arange(n + 1, dtype=np.uint64) * np.uint64(64)
    out = np.full((n, 64), 0xA5, dtype=np.uint8)
    assert L.zkt_sha512_batch(p_(buf), p_(off), n, p_(out)) == ZKT_OK
    raw, got = buf.tobytes(), out.tobytes()
    assert all(got[64 * i:64 * i + 64] == hashlib.sha512(raw[64 * i:64 * i + 64]).digest() for i in range(n)), ("sha512", n)


def signed_set():
    """8 (msg, sig, pub, want): four signatures of the model over 64-byte messages, and each of them again with the lowest bit of S flipped"""
    r, out = M._Rng(77), []
    for _ in range(4):
        prv, msg = r.bytes(32), r.bytes(64)
        pub, sig = M.gen_pub_key(prv), M.sign(msg, prv)
        bad = sig[:32] + bytes([sig[32] ^ 1]) + sig[33:]
        out += [(msg, sig, pub, M.verify(sig, pub, msg)), (msg, bad, pub, M.verify(bad, pub, msg))]
    assert [w for _, _, _, w in out] == [True, False] * 4
    return out


SIGNED = signed_set()


def ed_verify(n):
    case = [SIGNED[(3 * i) % 8] for i in range(n)]
    buf, off = M.pack_messages([c[0] for c in case])
    sigs = np.frombuffer(b"".join(c[1] for c in case), dtype=np.uint8).copy(); pubs = np.frombuffer(b"".join(c[2] for c in case), dtype=np.uint8).copy()
    ok = np.full(n, 7, np.uint32)
    assert L.zkt_ed25519_verify_batch(p_(buf), p_(off), p_(sigs), p_(pubs), n, p_(ok)) == ZKT_OK
    assert ok.tolist() == [int(c[3]) for c in case], ("ed25519_verify", n)


# before zkt_init: the digest forms report the missing device before the missing digests
one = np.zeros(16, np.uint64)
assert L.zkt_ecdsa_sign_digest_batch(None, p_(one), p_(one), 1, p_(one), None) == ZKT_ERR_DEVICE
assert L.zkt_ecdsa_verify_digest_batch(None, p_(one), p_(one), 1, p_(one)) == ZKT_ERR_DEVICE
assert L.zkt_init(-1) == ZKT_OK
assert L.zkt_ecdsa_sign_digest_batch(None, p_(one), p_(one), 1, p_(one), None) == ZKT_ERR_SHAPE
assert L.zkt_ecdsa_verify_digest_batch(None, p_(one), p_(one), 1, p_(one)) == ZKT_ERR_SHAPE
for step, n in [(fr_mul, 1), (ed_verify, 1), (sha512, 1), (fr_mul, 20000), (ed_verify, 256), (sha512, 30000), (ed_verify, 65), (fr_mul, 200000), (ed_verify, 256),
                (sha512, 200000), (ed_verify, 64), (fr_mul, 200000), (sha512, 30000), (fr_mul, 20000), (ed_verify, 3), (sha512, 1), (fr_mul, 1), (ed_verify, 1)]:
    step(n)
    print(step.__name__, n, "ok", flush=True)
L.zkt_shutdown()
print("ok")
