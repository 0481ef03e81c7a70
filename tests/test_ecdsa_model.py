"""The python-integer ECDSA model (tests/ecdsa_model.py) reproduces every scenario the reference tests (ecdsa.rs:142-317), hashlib agrees with the digests the
reference asserts (tests/golden/sha256_kats.json, sha256.rs:93-141), and the case list holds the constructed branches with the decisions the model's derivation gives."""
import hashlib, json, os
import pytest
from zkt_testlib import GOLDEN, SECP_N as N, SECP_P as P, SECP_GEN as G, SplitMix64, py_secp_mul
import ecdsa_model as M

MSG = M.digest([1, 2, 3])


def _signed(d, z, seed):
    rng = SplitMix64(seed)
    while True:
        sg = M.sign(z, d, 1 + rng.below(N - 1))
        if sg != M.RETRY: return sg


def test_hashlib_agrees_with_the_golden_digests():
    kats = json.load(open(os.path.join(GOLDEN, "sha256_kats.json")))["kats"]
    assert len(kats) == 5
    for k in kats:
        msg = bytes.fromhex(k["msg_hex"]) if "msg_hex" in k else bytes.fromhex(k["repeat"]["byte_hex"]) * k["repeat"]["count"]
        d = hashlib.sha256(msg).digest()
        assert d.hex() == k["digest"] and hashlib.sha256(d).hexdigest() == k["double"], k["name"]
    assert [k["repeat"]["count"] for k in kats if "repeat" in k] == [1000000]


def test_model_group_arithmetic_against_the_affine_model():
    rng = SplitMix64(3)
    for k in (1, 2, 3, N - 1, N - 2, rng.below(N), rng.below(N)):
        assert M.mul(G, k) == py_secp_mul(G, k)
    assert M.mul(G, N) is None and M.mul(G, 0) is None and M.mul(None, 5) is None


def test_sign_verify_bad_pub_key():                                    # ecdsa.rs:142-174
    d = 0x1234567 ; r, s = _signed(d, MSG, 1)
    x = M.gen_pub_key(d)[0]
    assert M.verify(MSG, r, s, (x, x)) is False


def test_sign_verify_inf_pub_key():                                    # :176-192
    r, s = _signed(99, MSG, 2)
    assert M.verify(MSG, r, s, None) is False


def test_sign_verify_sig_r_out_of_range():                             # :194-224
    d = 4242; r, s = _signed(d, MSG, 3); Q = M.gen_pub_key(d)
    assert M.verify(MSG, r, s, Q) is True
    assert M.verify(MSG, N, s, Q) is False and M.verify(MSG, 0, s, Q) is False


def test_sign_verify_sig_s_out_of_range():                             # :226-256
    d = 4243; r, s = _signed(d, MSG, 4); Q = M.gen_pub_key(d)
    assert M.verify(MSG, r, N, Q) is False and M.verify(MSG, r, 0, Q) is False


def test_sign_verify_all_good():                                       # :258-274 — private key 1234 over [1, 2, 3]
    r, s = _signed(1234, MSG, 5)
    assert M.verify(MSG, r, s, M.gen_pub_key(1234)) is True


def test_sign_verify_bad_priv_key():                                   # :276-295
    r, s = _signed(777, MSG, 6)
    assert M.verify(MSG, r, s, M.gen_pub_key(778)) is False


def test_sign_verify_different_message():                              # :297-317
    r, s = _signed(555, MSG, 7)
    assert M.verify(M.digest([1, 2, 3, 4]), r, s, M.gen_pub_key(555)) is False


def test_sign_retry_branches_and_reductions():
    assert M.sign(MSG, 5, 0) == M.RETRY and M.sign(MSG, 5, N) == M.RETRY                       # :61
    k = 12345; r = M.mul(G, k)[0] % N
    d = (-(int.from_bytes(MSG, "big") % N) * pow(r, -1, N)) % N
    assert M.sign(MSG, d, k) == M.RETRY                                                        # :77
    assert M.sign(MSG, d + N, k + N) == M.RETRY and M.sign(MSG, 7 + N, 9 + N) == M.sign(MSG, 7, 9)      # reduced on load
    assert sum(M.sign(*t) == M.RETRY for t in M.sign_cases()) == 4


def test_case_list_holds_every_kind_with_the_derived_decision():
    cases = M.verify_cases()
    assert len(cases) <= 150                                           # four rotations stay within the 600 elements of the GPU batch
    got = {}
    for c in cases:
        got.setdefault(c["kind"].split(" d=")[0], set()).add(M.verify(c["z"], c["r"], c["s"], c["Q"]))
    want = {"valid": {True}, "flip r": {False}, "flip s": {False}, "flip digest": {False}, "flip Q.x": {False}, "other key": {False}, "other message": {False},
            "Q at infinity": {False}, "Q=(x,x)": {False}, "Q.x=2^256-1": {False}, "doubling": {True}, "cancellation": {False}, "wrap x=n+2": {True},
            "wrap x=n+2 r+1": {False}, "valid, Q.x + p stored": {True}, "invalid, Q.x + p stored": {False}, "invalid": {False}, "valid Q=-G": {True}}
    for k, v in want.items():
        assert got.get(k) == v, (k, got.get(k))
    assert any(k.startswith("wrap mirror") and v == {True} for k, v in got.items())
    for k, v in got.items():
        if k.startswith(("r=", "s=")): assert v == {False}, k
        if k.startswith("valid digest"): assert v == {True}, k
    # the chosen keys are the issue's: G, -G, 2G, 3G, (n-1)G, (n-2)G
    keys = {c["Q"] for c in cases if c["Q"] is not None}
    for d in (1, 2, 3, N - 1, N - 2):
        assert M.gen_pub_key(d) in keys
    assert M.neg(G) in keys and M.gen_pub_key(N - 1) == M.neg(G)


def test_constructed_branches_are_what_they_claim():
    """doubling: u1 G == u2 Q; cancellation: u1 G == -(u2 Q); wrap: x(u1 G + u2 Q) = n + 2 >= n and r = 2"""
    from zkt_testlib import py_secp_add
    for c in M.verify_cases():
        kind = c["kind"]
        if kind not in ("doubling", "cancellation") and not kind.startswith("wrap x=n+2") or kind.endswith("r+1"): continue
        z = int.from_bytes(c["z"], "big") % N; w = pow(c["s"], -1, N)
        a, b = M.mul(G, z * w % N), M.mul(c["Q"], c["r"] * w % N)
        if kind == "doubling": assert a == b
        elif kind == "cancellation": assert a == M.neg(b) and py_secp_add(a, b) is None
        else:
            R = py_secp_add(a, b)
            assert R[0] == N + 2 and c["r"] == 2 and M.on_curve(*R)


def test_n_times_every_public_key_of_the_list_is_infinity():
    """ecdsa.rs:102, which verify() and the kernel omit: it holds for every on-curve key (cofactor 1)"""
    for c in M.verify_cases()[::7]:
        Q = c["Q"]
        if Q is None or not M.on_curve(Q[0] % P, Q[1] % P): continue
        assert M.mul((Q[0] % P, Q[1] % P), N) is None
