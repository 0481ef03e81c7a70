"""tests/ed25519_model.py against the RFC 8032 vectors of the reference's own tests, against itself (the reference's affine chain and the fast projective
form), and the content of the case list the host-check and GPU tests share.  No GPU, no library."""
import os, subprocess, sys
import ed25519_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_model_reproduces_the_five_vectors_with_the_reference_chain():
    vs = M.vectors()
    assert len(vs) == 5 and sorted(len(v["msg_hex"]) for v in vs) == [0, 1, 2, 64, 1023]
    for v in vs:
        assert M.gen_pub_key(v["prv"], chain=True) == v["pub"], v["name"]
        assert M.sign(v["msg_hex"], v["prv"], chain=True) == v["sig"], v["name"]
        assert M.sign(v["msg_hex"], v["prv"]) == v["sig"]
    assert M.verify(vs[0]["sig"], vs[0]["pub"], vs[0]["msg_hex"], chain=True)


def test_chain_and_fast_forms_agree_on_curve():
    cases = [c for c in M.verify_cases() if c["on_curve"]]
    kinds = ("vector", "honest", "flip S", "order-4 key as bytes of q", "order-4 key canonical", "mixed-order key", "mixed-order R", "r=0 y=q+1")
    picked = [next(c for c in cases if c["kind"].startswith(k)) for k in kinds]
    assert len(picked) == 8
    for c in picked:
        assert M.verify(c["sig"], c["pub"], c["msg"], chain=True) == M.verify(c["sig"], c["pub"], c["msg"], chain=False) == c["want"], c["kind"]
    T8 = M.torsion8()
    assert M.on_curve(T8) and M.fast_mul(T8, 8) == M.ZERO and M.fast_mul(T8, 4) != M.ZERO
    assert M.chain_mul(T8, 8) == M.ZERO and M.chain_mul(M.B, M.L) == M.ZERO and M.fast_mul(M.B, M.L) == M.ZERO


def test_case_list_holds_every_kind_with_its_decision():
    cases = M.verify_cases()
    def of(prefix): return [c for c in cases if c["kind"].startswith(prefix)]
    assert len(of("vector")) == 5 and all(c["want"] for c in of("vector"))
    assert len(of("honest")) == 64 and all(c["want"] for c in of("honest"))
    for k in ("flip R", "flip S", "flip key", "flip message", "wrong key", "wrong message"):
        assert of(k) and not any(c["want"] for c in of(k)), k
    assert [(c["kind"], c["want"]) for c in of("S=")] == [(k, False) for k in ("S=0", "S=l-1", "S=l", "S=S+l", "S=2^256-1")]
    assert int.from_bytes(of("S=S+l")[0]["sig"][32:], "little") - M.L == int.from_bytes(cases[5 + 3]["sig"][32:], "little")      # S_valid + l still fits 256 bits
    for k in ("r=0 canonical", "r=0 y=q+1", "r=0 sign bit on x=0"):
        (c,) = of(k); assert c["want"] and M.decode_point(c["sig"][:32]) == M.ZERO, k
    assert len({c["sig"][:32] for c in of("r=0")}) == 3
    for k in ("order-4 key as bytes of q", "order-4 key canonical", "mixed-order key"):
        got = [c["want"] for c in of(k)]
        assert len(got) == 16 and True in got and False in got, (k, got)
    assert M.decode_point(of("order-4 key as bytes of q")[0]["pub"]) == M.decode_point(of("order-4 key canonical")[0]["pub"])
    assert M.fast_mul(M.decode_point(of("order-4 key canonical")[0]["pub"]), 4) == M.ZERO
    # cofactored verification (8 S B == 8 R + 8 k A) would accept every mixed-order signature; the reference multiplies A by 8k mod l
    for c in of("mixed-order key"):
        S = int.from_bytes(c["sig"][32:], "little"); R = M.decode_point(c["sig"][:32]); A = M.decode_point(c["pub"])
        k = int.from_bytes(M.H(M.encode_point(R) + c["pub"] + c["msg"]), "little") % M.L
        assert M.fast_mul(M.B, 8 * S) == M.fast_add(M.fast_mul(R, 8), M.fast_mul(A, 8 * k))
        assert c["want"] == ((8 * k) % M.L % 8 == 0)
    assert len(of("mixed-order R")) == 3 and all(c["want"] for c in of("mixed-order R"))
    assert all(M.fast_mul(M.decode_point(c["sig"][:32]), M.L) != M.ZERO for c in of("mixed-order R"))


def test_every_off_curve_case_decides_false_without_a_panic():
    off = [c for c in M.verify_cases() if not c["on_curve"]]
    assert 6 <= len(off) <= 24
    assert {"off-curve R", "off-curve A"} <= {c["kind"] for c in off}
    for c in off:
        assert M.verify(c["sig"], c["pub"], c["msg"], chain=True) is False, c["kind"]      # a ZeroDivisionError here is the reference's panic
        assert c["want"] is False


def test_decode_cases_hold_the_named_edges():
    want = {e: M.decode_want(e) for e in M.decode_cases()}
    Q = M.Q
    assert want[(Q + 1).to_bytes(32, "little")] == (0, 1, True)                     # y = q + 1: the point (0, 1)
    x, y, on = want[Q.to_bytes(32, "little")]; assert y == 0 and on and x * x % Q == Q - 1      # y = q: an order-4 point (+-I, 0)
    assert want[(1 | 1 << 255).to_bytes(32, "little")] == (0, 1, True)              # y = 1 with the sign bit set: x stays 0
    assert want[(0).to_bytes(32, "little")][1:] == (0, True) and want[(Q - 1).to_bytes(32, "little")][:2] == (0, Q - 1)
    assert want[b"\xff" * 32][1] == (2 ** 255 - 1) % Q                               # 2^255 - 1 after masking
    flags = [w[2] for w in want.values()]
    assert 15 < sum(flags) < len(flags) - 15


def test_constants_header_is_what_the_generator_writes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_ed25519_constants.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    hdr = open(os.path.join(ROOT, "zk-toolkit_amd", "csrc", "ed25519_constants.h")).read()
    def words(v): return ",".join("0x%08xu" % ((v >> (32 * i)) & 0xFFFFFFFF) for i in range(8))
    for v in (M.Q, M.D, 2 * M.D % M.Q, M.I, M.B[0], M.B[1], M.L):
        assert words(v) in hdr
