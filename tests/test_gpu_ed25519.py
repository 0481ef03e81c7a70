"""Batched SHA-512 and Ed25519 on the GPU (csrc/zkt_ed25519.hip) through the C ABI, against hashlib and the python-integer model of tests/ed25519_model.py
(sha512.rs:91-97, ed25519_sha512.rs:85-186).  The model's keys, signatures and decisions are computed once per module and shared."""
import hashlib, importlib, json, math, os
import numpy as np
import pytest
from zkt_testlib import *
import ed25519_model as M

pytestmark = pytest.mark.gpu
zk = importlib.import_module("zk-toolkit_amd")
SHA_LENGTHS = (0, 1, 3, 111, 112, 113, 127, 128, 129, 239, 240, 256, 1000)


@pytest.fixture(scope="module")
def L():
    zk.init()
    return zk.lib()


def _sha(L, msgs):
    buf, off = M.pack_messages(msgs)
    out = np.full((len(msgs), 64), 0xA5, dtype=np.uint8)
    zk.check(L.zkt_sha512_batch(buf.ctypes.data, ptr(off), len(msgs), out.ctypes.data))
    return [out[i].tobytes() for i in range(len(msgs))]


def _messages(n, seed, lengths=SHA_LENGTHS):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [rng.integers(0, 256, size=lengths[i % len(lengths)], dtype=np.uint8).tobytes() for i in range(n)]


# ---- SHA-512 -----------------------------------------------------------------------------------------------------------------------------------------
def _kats():
    with open(os.path.join(GOLDEN, "sha512_kats.json")) as f:
        return json.load(f)["kats"]


def test_sha512_golden_kats_and_their_double_hashes(L):
    small = [k for k in _kats() if "msg_hex" in k]
    assert len(small) == 4
    first = _sha(L, [bytes.fromhex(k["msg_hex"]) for k in small])
    assert [d.hex() for d in first] == [k["digest"] for k in small]
    assert [d.hex() for d in _sha(L, first)] == [k["double"] for k in small]


def test_sha512_one_million_a_alone(L):
    (k,) = [k for k in _kats() if "repeat" in k]
    msg = bytes.fromhex(k["repeat"]["byte_hex"]) * k["repeat"]["count"]
    (d,) = _sha(L, [msg])
    assert d.hex() == k["digest"]
    assert _sha(L, [d])[0].hex() == k["double"]


def test_sha512_130_messages_every_length_and_alignment(L):
    msgs = [b""] + _messages(63, 1) + [b""] + _messages(64, 2) + [b""]        # an empty message first, between two others, and last
    assert len(msgs) == 130
    starts = np.cumsum([0] + [len(m) for m in msgs[:-1]])
    assert {int(s) % 8 for s in starts} == set(range(8))
    assert {int(s) % 8 for s, m in zip(starts, msgs) if len(m) >= 128} == set(range(8))      # whole blocks inside a message at every alignment
    assert _sha(L, msgs) == [hashlib.sha512(m).digest() for m in msgs]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sha512_batch_sizes(L, n):
    msgs = _messages(n, 100 + n)
    assert _sha(L, msgs) == [hashlib.sha512(m).digest() for m in msgs]


def test_sha512_shapes(L):
    buf, off = M.pack_messages([b"abc", b"de"])
    out = np.zeros((2, 64), np.uint8)
    assert L.zkt_sha512_batch(buf.ctypes.data, None, 2, out.ctypes.data) == ZKT_ERR_SHAPE
    assert L.zkt_sha512_batch(buf.ctypes.data, ptr(off), 2, None) == ZKT_ERR_SHAPE
    assert L.zkt_sha512_batch(None, ptr(off), 2, out.ctypes.data) == ZKT_ERR_SHAPE
    assert L.zkt_sha512_batch(buf.ctypes.data, ptr(off), 0, out.ctypes.data) == ZKT_OK
    bad = np.array([0, 3, 1, 5], dtype=np.uint64)                                 # element 1 ends before it starts: an empty message
    out3 = np.zeros((3, 64), np.uint8)
    zk.check(L.zkt_sha512_batch(buf.ctypes.data, ptr(bad), 3, out3.ctypes.data))
    assert [out3[i].tobytes() for i in range(3)] == [hashlib.sha512(m).digest() for m in (b"abc", b"", b"bcde")]
    assert L.zkt_sha512_batch(None, ptr(np.array([0, 5, 0], dtype=np.uint64)), 2, out.ctypes.data) == ZKT_ERR_SHAPE      # the extent, not offsets[n]
    zk.check(L.zkt_sha512_batch(None, ptr(np.zeros(3, dtype=np.uint64)), 2, out.ctypes.data))                              # no byte named: NULL is fine
    assert out[0].tobytes() == hashlib.sha512(b"").digest() and out[1].tobytes() == hashlib.sha512(b"").digest()


# ---- decode ------------------------------------------------------------------------------------------------------------------------------------------
def test_decode_257_strings_x_y_and_flag(L):
    encs = M.decode_cases(n_random=257 - 15)
    assert len(encs) == 257
    enc = np.frombuffer(b"".join(encs), dtype=np.uint8).copy()
    xy = np.full((257, 8), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64); on = np.full(257, 7, np.uint32)
    zk.check(L.zkt_ed25519_decode_batch(enc.ctypes.data, 257, ptr(xy), on.ctypes.data))
    want = [M.decode_want(e) for e in encs]
    got = [(limbs_to_int(xy[i, :4]), limbs_to_int(xy[i, 4:]), bool(on[i])) for i in range(257)]
    assert got == want
    assert 80 < int(on.sum()) < 177 and set(on.tolist()) == {0, 1}
    assert L.zkt_ed25519_decode_batch(None, 2, ptr(xy), on.ctypes.data) == ZKT_ERR_SHAPE
    assert L.zkt_ed25519_decode_batch(enc.ctypes.data, 2, None, on.ctypes.data) == ZKT_ERR_SHAPE
    assert L.zkt_ed25519_decode_batch(enc.ctypes.data, 2, ptr(xy), None) == ZKT_ERR_SHAPE
    assert L.zkt_ed25519_decode_batch(enc.ctypes.data, 0, ptr(xy), on.ctypes.data) == ZKT_OK


# ---- public keys and signing -------------------------------------------------------------------------------------------------------------------------
def _pubs(L, prvs):
    n = len(prvs)
    prv = np.frombuffer(b"".join(prvs), dtype=np.uint8).copy(); pub = np.full((n, 32), 0xA5, np.uint8)
    zk.check(L.zkt_ed25519_public_keys_batch(prv.ctypes.data, n, pub.ctypes.data))
    return [pub[i].tobytes() for i in range(n)]


def _sign(L, prvs, msgs):
    n = len(prvs)
    prv = np.frombuffer(b"".join(prvs), dtype=np.uint8).copy(); sig = np.full((n, 64), 0xA5, np.uint8)
    buf, off = M.pack_messages(msgs)
    zk.check(L.zkt_ed25519_sign_batch(buf.ctypes.data, ptr(off), prv.ctypes.data, n, sig.ctypes.data))
    return [sig[i].tobytes() for i in range(n)]


def _verify(L, msgs, sigs, pubs):
    n = len(msgs)
    buf, off = M.pack_messages(msgs)
    s = np.frombuffer(b"".join(sigs), dtype=np.uint8).copy(); p = np.frombuffer(b"".join(pubs), dtype=np.uint8).copy()
    ok = np.full(n, 7, np.uint32)
    assert L.zkt_ed25519_verify_batch(buf.ctypes.data, ptr(off), s.ctypes.data, p.ctypes.data, n, ok.ctypes.data) == ZKT_OK      # never a per-element error
    return ok


def test_the_five_vectors_are_exact(L):
    vs = M.vectors()
    assert len(vs) == 5 and max(len(v["msg_hex"]) for v in vs) == 1023
    assert _pubs(L, [v["prv"] for v in vs]) == [v["pub"] for v in vs]
    assert _sign(L, [v["prv"] for v in vs], [v["msg_hex"] for v in vs]) == [v["sig"] for v in vs]
    assert _verify(L, [v["msg_hex"] for v in vs], [v["sig"] for v in vs], [v["pub"] for v in vs]).tolist() == [1] * 5


@pytest.fixture(scope="module")
def signed():
    """257 random (prv, msg, pub, sig) from the model, message lengths cycling through the block edges of prefix‖msg and R‖A‖msg"""
    rng = M._Rng(257)
    prvs = [rng.bytes(32) for _ in range(257)]
    msgs = _messages(257, 9, M.MSG_LENGTHS)
    return {"prv": prvs, "msg": msgs, "pub": [M.gen_pub_key(p) for p in prvs], "sig": [M.sign(m, p) for m, p in zip(msgs, prvs)]}


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_keys_and_signatures_match_the_model_and_verify(L, signed, n):
    lo = 257 - n                                                                   # the tail: n = 1 signs the last message, every n starts at another length
    prvs, msgs = signed["prv"][lo:], signed["msg"][lo:]
    assert _pubs(L, prvs) == signed["pub"][lo:]
    sigs = _sign(L, prvs, msgs)
    assert sigs == signed["sig"][lo:]
    assert _verify(L, msgs, sigs, signed["pub"][lo:]).tolist() == [1] * n


def test_key_and_sign_shapes(L):
    prv = np.zeros(64, np.uint8); out = np.zeros(128, np.uint8)
    buf, off = M.pack_messages([b"ab", b"c"])
    assert L.zkt_ed25519_public_keys_batch(None, 2, out.ctypes.data) == ZKT_ERR_SHAPE
    assert L.zkt_ed25519_public_keys_batch(prv.ctypes.data, 2, None) == ZKT_ERR_SHAPE
    assert L.zkt_ed25519_public_keys_batch(prv.ctypes.data, 0, out.ctypes.data) == ZKT_OK
    S = L.zkt_ed25519_sign_batch
    assert S(buf.ctypes.data, None, prv.ctypes.data, 2, out.ctypes.data) == ZKT_ERR_SHAPE
    assert S(buf.ctypes.data, ptr(off), None, 2, out.ctypes.data) == ZKT_ERR_SHAPE
    assert S(buf.ctypes.data, ptr(off), prv.ctypes.data, 2, None) == ZKT_ERR_SHAPE
    assert S(None, ptr(off), prv.ctypes.data, 2, out.ctypes.data) == ZKT_ERR_SHAPE
    assert S(None, ptr(np.array([0, 5, 0], dtype=np.uint64)), prv.ctypes.data, 2, out.ctypes.data) == ZKT_ERR_SHAPE
    assert S(buf.ctypes.data, ptr(off), prv.ctypes.data, 0, out.ctypes.data) == ZKT_OK
    # NULL msgs with all-zero offsets: two empty messages; and an element that ends before it starts signs the empty message too
    zk.check(S(None, ptr(np.zeros(3, np.uint64)), prv.ctypes.data, 2, out.ctypes.data))
    assert out[:64].tobytes() == M.sign(b"", bytes(32))
    zk.check(S(buf.ctypes.data, ptr(np.array([2, 1, 3], dtype=np.uint64)), prv.ctypes.data, 2, out.ctypes.data))
    assert out[:64].tobytes() == M.sign(b"", bytes(32)) and out[64:].tobytes() == M.sign(b"bc", bytes(32))


# ---- verification ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mix():
    """the model's case list three times over in a stride order coprime to its length, so that every case sits on three lanes of different waves; the
    constructed cases are then planted on the lanes around the first three wave boundaries.  Decisions come from the model, once per case."""
    cases = M.verify_cases()
    n = len(cases)
    stride = next(s for s in range(41, 200) if math.gcd(s, n) == 1)
    order = [(i * stride) % n for i in range(3 * n)]
    pick = lambda word, w: next(i for i, c in enumerate(cases) if c["kind"].startswith(word) and c["want"] == w)
    planted = [pick("r=0 canonical", True), pick("r=0 y=q+1", True), pick("r=0 sign bit", True), pick("order-4 key as bytes of q", True), pick("order-4 key canonical", False),
               pick("mixed-order key", True), pick("mixed-order key", False), pick("mixed-order R", True), pick("off-curve R", False)]
    for slot, ci in zip([63, 64, 65, 127, 128, 129, 191, 192, 193], planted):
        order[slot] = ci
    assert set(order) == set(range(n))
    batch = [cases[i] for i in order]
    buf, off, sigs, pubs = M.pack_cases(batch)
    return {"cases": batch, "want": np.array([c["want"] for c in batch], dtype=np.uint32), "buf": buf, "off": off, "sigs": sigs, "pubs": pubs}


def _window(mix, lo, n):
    """elements lo .. lo+n of the mix as a batch of their own (offsets rebased)"""
    off = mix["off"][lo:lo + n + 1] - mix["off"][lo]
    buf = mix["buf"][int(mix["off"][lo]):int(mix["off"][lo + n])]
    return np.ascontiguousarray(buf if len(buf) else np.zeros(1, np.uint8)), np.ascontiguousarray(off), np.ascontiguousarray(mix["sigs"][lo:lo + n]), np.ascontiguousarray(mix["pubs"][lo:lo + n])


def test_verify_the_mix_element_by_element(L, mix):
    n = len(mix["want"])
    ok = np.full(n, 7, np.uint32)
    assert L.zkt_ed25519_verify_batch(mix["buf"].ctypes.data, ptr(mix["off"]), mix["sigs"].ctypes.data, mix["pubs"].ctypes.data, n, ok.ctypes.data) == ZKT_OK
    bad = [(i, mix["cases"][i]["kind"], int(ok[i]), int(mix["want"][i])) for i in range(n) if ok[i] != mix["want"][i]]
    assert not bad, bad[:10]
    assert mix["want"].sum() > 150 and (mix["want"] == 0).sum() > 150


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_verify_batch_sizes(L, mix, n):
    lo = 40 if n > 1 else 64                                              # windows that span the planted lanes
    buf, off, sigs, pubs = _window(mix, lo, n)
    ok = np.full(n, 7, np.uint32)
    zk.check(L.zkt_ed25519_verify_batch(buf.ctypes.data, ptr(off), sigs.ctypes.data, pubs.ctypes.data, n, ok.ctypes.data))
    assert (ok == mix["want"][lo:lo + n]).all()


def test_verify_dev_form_equals_host_form(L, mix):
    import torch
    n = len(mix["want"])
    d_buf = torch.from_numpy(mix["buf"].copy()).cuda()
    d_off = torch.from_numpy(mix["off"].view(np.int64).copy()).cuda()
    d_sig = torch.from_numpy(mix["sigs"].copy()).cuda()
    d_pub = torch.from_numpy(mix["pubs"].copy()).cuda()
    d_ok = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        zk.check(L.zkt_ed25519_verify_batch_dev(d_buf.data_ptr(), d_off.data_ptr(), d_sig.data_ptr(), d_pub.data_ptr(), n, d_ok.data_ptr(), stream.cuda_stream))
    stream.synchronize()
    assert (d_ok.cpu().numpy().astype(np.uint32) == mix["want"]).all()


def test_verify_shapes(L, mix):
    buf, off, sigs, pubs = _window(mix, 0, 2)
    ok = np.zeros(2, np.uint32)
    V = L.zkt_ed25519_verify_batch
    assert V(buf.ctypes.data, None, sigs.ctypes.data, pubs.ctypes.data, 2, ok.ctypes.data) == ZKT_ERR_SHAPE
    assert V(buf.ctypes.data, ptr(off), None, pubs.ctypes.data, 2, ok.ctypes.data) == ZKT_ERR_SHAPE
    assert V(buf.ctypes.data, ptr(off), sigs.ctypes.data, None, 2, ok.ctypes.data) == ZKT_ERR_SHAPE
    assert V(buf.ctypes.data, ptr(off), sigs.ctypes.data, pubs.ctypes.data, 2, None) == ZKT_ERR_SHAPE
    assert V(None, ptr(np.array([0, 5, 0], dtype=np.uint64)), sigs.ctypes.data, pubs.ctypes.data, 2, ok.ctypes.data) == ZKT_ERR_SHAPE
    assert V(buf.ctypes.data, ptr(off), sigs.ctypes.data, pubs.ctypes.data, 0, ok.ctypes.data) == ZKT_OK
    D = L.zkt_ed25519_verify_batch_dev
    one = 64                                                              # any non-null address: a shape error is decided before anything is read
    assert D(one, None, one, one, 2, one, None) == ZKT_ERR_SHAPE
    assert D(one, one, None, one, 2, one, None) == ZKT_ERR_SHAPE
    assert D(one, one, one, None, 2, one, None) == ZKT_ERR_SHAPE
    assert D(one, one, one, one, 2, None, None) == ZKT_ERR_SHAPE
    assert D(one, one, one, one, 0, one, None) == ZKT_OK
