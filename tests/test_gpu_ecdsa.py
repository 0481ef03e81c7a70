"""Batched SHA-256 and secp256k1 ECDSA on the GPU (csrc/zkt_ecdsa.hip) against hashlib and the python-integer model of tests/ecdsa_model.py
(sha256.rs:75-81, ecdsa.rs:33-135).  The model's decisions and signatures are computed once per module and shared.

Not reachable by any test: the r == 0 retry of signing (ecdsa.rs:67) needs a nonce k with x(k G) = n, and no such k is known."""
import ctypes, hashlib, importlib, json, os
import numpy as np
import pytest
from zkt_testlib import *
import ecdsa_model as M

pytestmark = pytest.mark.gpu
zk = importlib.import_module("zk-toolkit_amd")
SHA_LENGTHS = (0, 1, 3, 55, 56, 57, 63, 64, 65, 119, 120, 128, 1000)


@pytest.fixture(scope="module")
def L():
    zk.init()
    return zk.lib()


def _pack(msgs):
    off = np.zeros(len(msgs) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    buf = np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8).copy()
    return buf, off


def _sha(L, msgs):
    buf, off = _pack(msgs)
    out = np.full((len(msgs), 32), 0xA5, dtype=np.uint8)
    zk.check(L.zkt_sha256_batch(buf.ctypes.data, ptr(off), len(msgs), out.ctypes.data))
    return [out[i].tobytes() for i in range(len(msgs))]


def _messages(n, seed):
    """n messages whose lengths cycle through SHA_LENGTHS, laid out back to back: the odd lengths move the starts over all four alignments"""
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = [SHA_LENGTHS[i % len(SHA_LENGTHS)] for i in range(n)]
    return [rng.integers(0, 256, size=l, dtype=np.uint8).tobytes() for l in lens]


# ---- SHA-256 -----------------------------------------------------------------------------------------------------------------------------------------
def _kats():
    with open(os.path.join(GOLDEN, "sha256_kats.json")) as f:
        return json.load(f)["kats"]


def test_sha256_golden_kats_and_their_double_hashes(L):
    small = [k for k in _kats() if "msg_hex" in k]
    first = _sha(L, [bytes.fromhex(k["msg_hex"]) for k in small])
    assert [d.hex() for d in first] == [k["digest"] for k in small]
    assert [d.hex() for d in _sha(L, first)] == [k["double"] for k in small]


def test_sha256_one_million_a_alone(L):
    (k,) = [k for k in _kats() if "repeat" in k]
    msg = bytes.fromhex(k["repeat"]["byte_hex"]) * k["repeat"]["count"]
    (d,) = _sha(L, [msg])
    assert d.hex() == k["digest"]
    assert _sha(L, [d])[0].hex() == k["double"]


def test_sha256_130_messages_every_length_and_alignment(L):
    msgs = [b""] + _messages(63, 1) + [b""] + _messages(64, 2) + [b""]        # an empty message first, between two others, and last
    assert len(msgs) == 130
    starts = np.cumsum([0] + [len(m) for m in msgs[:-1]])
    for length in SHA_LENGTHS[1:]:
        seen = {int(s) % 4 for s, m in zip(starts, msgs) if len(m) == length}
        assert seen == {0, 1, 2, 3}, (length, seen)
    assert {int(s) % 4 for s in starts} == {0, 1, 2, 3}
    assert _sha(L, msgs) == [hashlib.sha256(m).digest() for m in msgs]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sha256_batch_sizes(L, n):
    msgs = _messages(n, 100 + n)
    assert _sha(L, msgs) == [hashlib.sha256(m).digest() for m in msgs]


def test_sha256_shapes(L):
    buf, off = _pack([b"abc", b"de"])
    out = np.zeros((2, 32), np.uint8)
    assert L.zkt_sha256_batch(buf.ctypes.data, None, 2, out.ctypes.data) == ZKT_ERR_SHAPE
    assert L.zkt_sha256_batch(buf.ctypes.data, ptr(off), 2, None) == ZKT_ERR_SHAPE
    assert L.zkt_sha256_batch(None, ptr(off), 2, out.ctypes.data) == ZKT_ERR_SHAPE
    assert L.zkt_sha256_batch(buf.ctypes.data, ptr(off), 0, out.ctypes.data) == ZKT_OK
    # an element whose end lies before its start is an empty message, as the BLS calls' hash treats it; its neighbours are unaffected
    bad = np.array([0, 3, 1, 5], dtype=np.uint64)
    out3 = np.zeros((3, 32), np.uint8)
    zk.check(L.zkt_sha256_batch(buf.ctypes.data, ptr(bad), 3, out3.ctypes.data))
    assert out3[0].tobytes() == hashlib.sha256(b"abc").digest() and out3[1].tobytes() == hashlib.sha256(b"").digest()
    assert out3[2].tobytes() == hashlib.sha256(b"bcde").digest()
    # a vector that ends at 0 but names bytes on the way needs the bytes: the check is on the extent, not on offsets[n]
    assert L.zkt_sha256_batch(None, ptr(np.array([0, 5, 0], dtype=np.uint64)), 2, out.ctypes.data) == ZKT_ERR_SHAPE
    zk.check(L.zkt_sha256_batch(None, ptr(np.zeros(3, dtype=np.uint64)), 2, out.ctypes.data))                      # no byte named: NULL is fine
    assert out[0].tobytes() == hashlib.sha256(b"").digest() and out[1].tobytes() == hashlib.sha256(b"").digest()


# ---- signing and public keys -------------------------------------------------------------------------------------------------------------------------
def _sign(L, triples, form="digest", retry=True):
    n = len(triples)
    sks, ks = ints_to_arr([t[1] for t in triples], 4), ints_to_arr([t[2] for t in triples], 4)
    sigs = np.full((n, 8), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    rt = np.full(n, 7, dtype=np.uint32) if retry else None
    rtp = rt.ctypes.data if retry else None
    if form == "digest":
        dig = np.frombuffer(b"".join(t[0] for t in triples), dtype=np.uint8).copy()
        rc = L.zkt_ecdsa_sign_digest_batch(dig.ctypes.data, ptr(sks), ptr(ks), n, ptr(sigs), rtp)
    else:
        buf, off = _pack([t[0] for t in triples])
        rc = L.zkt_ecdsa_sign_batch(buf.ctypes.data, ptr(off), ptr(sks), ptr(ks), n, ptr(sigs), rtp)
    return rc, sigs, rt


def _check_signatures(triples, sigs, rt):
    for i, (zb, d, k) in enumerate(triples):
        want = M.sign(zb, d, k)
        if want == M.RETRY:
            assert rt[i] == 1 and not sigs[i].any(), i
        else:
            assert rt[i] == 0 and (limbs_to_int(sigs[i, :4]), limbs_to_int(sigs[i, 4:])) == want, i


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_sign_and_public_keys_random(L, n):
    rng = SplitMix64(300 + n)
    triples = [(M._b32(rng.below(1 << 256)), rng.below(1 << 256), rng.below(1 << 256)) for _ in range(n)]      # d, k: any 256-bit value, reduced on load
    rc, sigs, rt = _sign(L, triples)
    assert rc == ZKT_OK
    _check_signatures(triples, sigs, rt)
    pks = np.zeros((n, 9), np.uint64)
    zk.check(L.zkt_ecdsa_public_keys_batch(ptr(ints_to_arr([t[1] for t in triples], 4)), n, ptr(pks)))
    assert (pks == secp_arr([M.gen_pub_key(t[1]) for t in triples])).all()


def test_sign_edges_and_retry(L):
    triples = M.sign_cases()
    wants = [M.sign(*t) for t in triples]
    assert sum(w == M.RETRY for w in wants) == 4                        # k = 0, k = n, two s == 0 constructions
    rc, sigs, rt = _sign(L, triples)
    assert rc == ZKT_OK                                                  # retries are reported per element, not as a status
    _check_signatures(triples, sigs, rt)
    # d in {0, n}: the key is the point at infinity
    pks = np.zeros((5, 9), np.uint64)
    zk.check(L.zkt_ecdsa_public_keys_batch(ptr(ints_to_arr([t[1] for t in triples[:5]], 4)), 5, ptr(pks)))
    assert (pks == secp_arr([M.gen_pub_key(t[1]) for t in triples[:5]])).all() and pks[0, 8] == 1 and pks[3, 8] == 1
    # a null retry: allowed only if no element needs one
    first = next(i for i, w in enumerate(wants) if w == M.RETRY)
    rc, _, _ = _sign(L, triples, retry=False)
    assert rc == ZKT_ERR_SHAPE and L.zkt_last_error_index() == first
    clean = [t for t, w in zip(triples, wants) if w != M.RETRY]
    rc, sigs2, _ = _sign(L, clean, retry=False)
    assert rc == ZKT_OK
    _check_signatures(clean, sigs2, np.zeros(len(clean), np.uint32))


def test_sign_message_form_is_the_digest_form_of_hashlib(L):
    rng = SplitMix64(41)
    msgs = [b""] + _messages(66, 9)
    by_msg = [(m, 1 + rng.below(M.N - 1), 1 + rng.below(M.N - 1)) for m in msgs]
    by_dig = [(hashlib.sha256(m).digest(), d, k) for m, d, k in by_msg]
    rc1, s1, r1 = _sign(L, by_msg, form="msg")
    rc2, s2, r2 = _sign(L, by_dig)
    assert rc1 == ZKT_OK and rc2 == ZKT_OK and (s1 == s2).all() and (r1 == r2).all()
    _check_signatures(by_dig, s1, r1)


def test_sign_and_public_key_shapes(L):
    a = np.zeros((1, 4), np.uint64); sig = np.zeros((1, 8), np.uint64); dig = np.zeros(32, np.uint8); pk = np.zeros((1, 9), np.uint64)
    assert L.zkt_ecdsa_sign_digest_batch(None, ptr(a), ptr(a), 1, ptr(sig), None) == ZKT_ERR_SHAPE
    assert L.zkt_ecdsa_sign_digest_batch(dig.ctypes.data, None, ptr(a), 1, ptr(sig), None) == ZKT_ERR_SHAPE
    assert L.zkt_ecdsa_sign_digest_batch(dig.ctypes.data, ptr(a), ptr(a), 1, None, None) == ZKT_ERR_SHAPE
    assert L.zkt_ecdsa_sign_digest_batch(dig.ctypes.data, ptr(a), ptr(a), 0, ptr(sig), None) == ZKT_OK
    assert L.zkt_ecdsa_sign_batch(None, None, ptr(a), ptr(a), 1, ptr(sig), None) == ZKT_ERR_SHAPE
    assert L.zkt_ecdsa_public_keys_batch(None, 1, ptr(pk)) == ZKT_ERR_SHAPE and L.zkt_ecdsa_public_keys_batch(ptr(a), 1, None) == ZKT_ERR_SHAPE
    assert L.zkt_ecdsa_public_keys_batch(ptr(a), 0, ptr(pk)) == ZKT_OK


# ---- verification ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mix():
    """one batch of 592 elements: the 148 cases of ecdsa_model.verify_cases() four times over in a stride-41 order (41 is coprime to 148), so that every case sits
    at four different lanes of four different waves; the constructed branches are then planted on lanes 63 / 64 / 65 of the first wave boundaries.
    Decisions come from the model, once per case."""
    cases = M.verify_cases()
    want_of = [M.verify(c["z"], c["r"], c["s"], c["Q"]) for c in cases]
    order = [(i * 41) % len(cases) for i in range(4 * len(cases))]
    pick = lambda word, w: next(i for i, c in enumerate(cases) if c["kind"].startswith(word) and want_of[i] == w)
    planted = [pick("doubling", True), pick("cancellation", False), pick("wrap x=n+", True), pick("wrap mirror", True), pick("valid d=1234", True), pick("Q at infinity", False),
               pick("r=", False), pick("valid digest 0xffff", True), pick("Q=(x,x)", False), pick("wrap x=n+2 r+1", False), pick("flip r", False), pick("valid, Q.x + p", True)]
    for slot, ci in zip([63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257], planted):
        order[slot] = ci
    assert len(order) <= 600 and set(order) == set(range(len(cases)))
    batch = [cases[i] for i in order]
    dig, sigs, pks = M.pack_cases(batch)
    return {"cases": batch, "want": np.array([want_of[i] for i in order], dtype=np.uint32), "dig": dig, "sigs": sigs, "pks": pks}


def _verify_digest(L, dig, sigs, pks):
    n = len(sigs)
    ok = np.full(n, 7, dtype=np.uint32)
    rc = L.zkt_ecdsa_verify_digest_batch(np.ascontiguousarray(dig).ctypes.data, ptr(np.ascontiguousarray(sigs)), ptr(np.ascontiguousarray(pks)), n, ok.ctypes.data)
    assert rc == ZKT_OK                                                  # never a per-element error
    return ok


def test_verify_the_mix_element_by_element(L, mix):
    ok = _verify_digest(L, mix["dig"], mix["sigs"], mix["pks"])
    bad = [(i, mix["cases"][i]["kind"], int(ok[i]), int(mix["want"][i])) for i in range(len(ok)) if ok[i] != mix["want"][i]]
    assert not bad, bad[:10]
    assert mix["want"].sum() > 100 and (mix["want"] == 0).sum() > 300


def test_verify_agrees_with_is_on_curve_on_the_same_bytes(L, mix):
    """a key that zkt_secp_is_on_curve_batch rejects (off the curve, or at infinity) never verifies; and the model's view of the loaded coordinates is that call's"""
    n = len(mix["pks"])
    on = np.zeros(n, np.uint32)
    zk.check(L.zkt_secp_is_on_curve_batch(ptr(mix["pks"]), on.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), n))
    model_on = [c["Q"] is not None and M.on_curve(c["Q"][0] % M.P, c["Q"][1] % M.P) for c in mix["cases"]]
    assert [bool(v) for v in on] == model_on
    assert not (mix["want"][on == 0]).any()
    assert any(c["Q"] is not None and c["Q"][0] >= M.P and on[i] == 1 for i, c in enumerate(mix["cases"]))      # a coordinate >= p that both calls accept
    assert any(c["Q"] is not None and c["Q"][0] >= M.P and on[i] == 0 for i, c in enumerate(mix["cases"]))      # and one that both reject


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_verify_batch_sizes(L, mix, n):
    lo = 40                                                              # a window of the mix that spans the planted lanes
    ok = _verify_digest(L, mix["dig"][lo:lo + n], mix["sigs"][lo:lo + n], mix["pks"][lo:lo + n])
    assert (ok == mix["want"][lo:lo + n]).all()


def test_verify_dev_form_equals_host_form(L, mix):
    import torch
    n = len(mix["sigs"])
    d_dig = torch.from_numpy(mix["dig"].copy()).cuda()
    d_sig = torch.from_numpy(mix["sigs"].view(np.int64).copy()).cuda()
    d_pk = torch.from_numpy(mix["pks"].view(np.int64).copy()).cuda()
    d_ok = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        zk.check(L.zkt_ecdsa_verify_digest_batch_dev(d_dig.data_ptr(), d_sig.data_ptr(), d_pk.data_ptr(), n, d_ok.data_ptr(), stream.cuda_stream))
    stream.synchronize()
    assert (d_ok.cpu().numpy().astype(np.uint32) == mix["want"]).all()


def _random_signed(n, seed):
    """n (message, r, s, Q) with every third one spoiled (s + 1, the next element's key, or another message)"""
    rng = SplitMix64(seed)
    msgs = _messages(n, seed)
    out = []
    for i, m in enumerate(msgs):
        d = 1 + rng.below(M.N - 1)
        r, s = M.sign(hashlib.sha256(m).digest(), d, 1 + rng.below(M.N - 1))
        Q = M.gen_pub_key(d)
        if i % 3 == 1: s = s % (M.N - 1) + 1
        if i % 6 == 5: Q = M.gen_pub_key(d + 1)
        out.append((m, r, s, Q))
    return out


def test_verify_message_form_is_the_digest_form_of_hashlib(L):
    items = [(b"", *_random_signed(2, 3)[1][1:])] + _random_signed(129, 4)      # _random_signed(2, .)[1] signs a one-byte message
    # element 0: the empty message under a signature made for another one (rejects), then one made for it
    d0 = 12345; r0, s0 = M.sign(hashlib.sha256(b"").digest(), d0, 999); items.insert(1, (b"", r0, s0, M.gen_pub_key(d0)))
    cases = [{"kind": "", "z": hashlib.sha256(m).digest(), "r": r, "s": s, "Q": Q} for m, r, s, Q in items]
    dig, sigs, pks = M.pack_cases(cases)
    want = np.array([M.verify(c["z"], c["r"], c["s"], c["Q"]) for c in cases], dtype=np.uint32)
    assert want[1] == 1 and want[0] == 0 and 40 < want.sum() < len(want)
    buf, off = _pack([it[0] for it in items])
    ok = np.full(len(items), 7, np.uint32)
    zk.check(L.zkt_ecdsa_verify_batch(buf.ctypes.data, ptr(off), ptr(sigs), ptr(pks), len(items), ok.ctypes.data))
    assert (ok == want).all()
    assert (_verify_digest(L, dig, sigs, pks) == want).all()


def test_verify_equals_the_composition_of_the_existing_calls(L):
    """the seven round trips the fused call replaces: s^-1, two sn products, two scalar multiplications, one addition, a host compare"""
    items = _random_signed(96, 8)
    n = len(items)
    cases = [{"kind": "", "z": hashlib.sha256(m).digest(), "r": r, "s": s, "Q": Q} for m, r, s, Q in items]
    dig, sigs, pks = M.pack_cases(cases)
    fused = _verify_digest(L, dig, sigs, pks)
    z = ints_to_arr([int.from_bytes(c["z"], "big") for c in cases], 4)
    r, s = np.ascontiguousarray(sigs[:, :4]), np.ascontiguousarray(sigs[:, 4:])
    w, u1, u2 = (np.zeros((n, 4), np.uint64) for _ in range(3))
    zk.check(L.zkt_sn_inv_batch(ptr(s), ptr(w), n))
    zk.check(L.zkt_sn_mul_batch(ptr(z), ptr(w), ptr(u1), n))
    zk.check(L.zkt_sn_mul_batch(ptr(r), ptr(w), ptr(u2), n))
    gens = secp_arr([SECP_GEN] * n)
    p1, p2, p3 = (np.zeros((n, 9), np.uint64) for _ in range(3))
    zk.check(L.zkt_secp_mul_batch(ptr(gens), ptr(u1), 4, ptr(p1), n))
    zk.check(L.zkt_secp_mul_batch(ptr(pks), ptr(u2), 4, ptr(p2), n))
    zk.check(L.zkt_secp_add_batch(ptr(p1), ptr(p2), ptr(p3), n))
    composed = np.array([p3[i, 8] == 0 and limbs_to_int(p3[i, :4]) % M.N == cases[i]["r"] for i in range(n)], dtype=np.uint32)
    assert (fused == composed).all() and 20 < fused.sum() < n


def test_verify_shapes(L, mix):
    dig, sigs, pks = mix["dig"][:2].copy(), mix["sigs"][:2].copy(), mix["pks"][:2].copy()
    ok = np.zeros(2, np.uint32)
    V = L.zkt_ecdsa_verify_digest_batch
    assert V(None, ptr(sigs), ptr(pks), 2, ok.ctypes.data) == ZKT_ERR_SHAPE
    assert V(dig.ctypes.data, None, ptr(pks), 2, ok.ctypes.data) == ZKT_ERR_SHAPE
    assert V(dig.ctypes.data, ptr(sigs), None, 2, ok.ctypes.data) == ZKT_ERR_SHAPE
    assert V(dig.ctypes.data, ptr(sigs), ptr(pks), 2, None) == ZKT_ERR_SHAPE
    assert V(dig.ctypes.data, ptr(sigs), ptr(pks), 0, ok.ctypes.data) == ZKT_OK
    buf, off = _pack([b"ab", b"c"])
    W = L.zkt_ecdsa_verify_batch
    assert W(buf.ctypes.data, None, ptr(sigs), ptr(pks), 2, ok.ctypes.data) == ZKT_ERR_SHAPE
    assert W(None, ptr(off), ptr(sigs), ptr(pks), 2, ok.ctypes.data) == ZKT_ERR_SHAPE
    assert W(buf.ctypes.data, ptr(off), ptr(sigs), ptr(pks), 0, ok.ctypes.data) == ZKT_OK
    assert W(None, ptr(np.array([0, 5, 0], dtype=np.uint64)), ptr(sigs), ptr(pks), 2, ok.ctypes.data) == ZKT_ERR_SHAPE
    assert L.zkt_ecdsa_verify_digest_batch_dev(None, None, None, 2, None, None) == ZKT_ERR_SHAPE
