"""Ed25519 over SHA-512 with python integers and hashlib: the checker of the Ed25519 tests.  The functions restate
src/building_block/curves/curve25519/ed25519_sha512.rs and affine_point.rs line by line (the cited lines).

Two group arithmetics:
  chain_mul / affine_add   the reference's own: the LSB-first chain of macros.rs:1-32 from the rational point (0, 1), the affine Edwards law of
                           affine_point.rs:119-143 with two divisions per addition; a division by zero raises ZeroDivisionError (the reference panics).
  fast_mul / fast_add      extended coordinates.  Used for points ON the curve only, where the law is complete and both give the same point
                           (tests/test_ed25519_model.py compares them).
verify() takes the chain whenever R or A decodes off the curve."""
import hashlib

Q = 2 ** 255 - 19
L = 2 ** 252 + 27742317777372353535851937790883648493
D = (-121665 * pow(121666, Q - 2, Q)) % Q                     # affine_point.rs:106-113
I = pow(2, (Q - 1) // 4, Q)                                   # :96-99


def H(b): return hashlib.sha512(bytes(b)).digest()
def inv(a):
    if a % Q == 0: raise ZeroDivisionError("Cannot find inverse of zero")
    return pow(a, Q - 2, Q)


def recover_x(y, odd):                                        # affine_point.rs:83-104
    xx = (y * y - 1) * inv(D * y * y + 1) % Q
    x = pow(xx, (Q + 3) // 8, Q)
    if x * x % Q != xx: x = x * I % Q                         # no second test
    if (x & 1) != odd: x = (-x) % Q
    return x


def on_curve(p): return (-p[0] * p[0] + p[1] * p[1] - 1 - D * p[0] * p[0] * p[1] * p[1]) % Q == 0
def decode_point(b):                                          # ed25519_sha512.rs:85-98
    b = bytearray(b)
    odd = b[31] >> 7
    b[31] &= 0x7F
    y = int.from_bytes(b, "little") % Q
    return (recover_x(y, odd), y)
def encode_point(p):                                          # :64-83
    return (p[1] | ((p[0] & 1) << 255)).to_bytes(32, "little")


BY = 4 * inv(5) % Q
B = (recover_x(BY, 0), BY)                                    # affine_point.rs:67-73
ZERO = (0, 1)                                                 # :167-173


def affine_add(p, q):                                         # affine_point.rs:119-143
    x1, y1 = p; x2, y2 = q
    x1y2, x2y1 = x1 * y2 % Q, x2 * y1 % Q
    t = x1y2 * x2y1 % Q
    return ((x1y2 + x2y1) * inv(1 + D * t) % Q, (y1 * y2 + x1 * x2) * inv(1 - D * t) % Q)


def chain_mul(p, n):                                          # macros.rs:9-23
    res, pw = ZERO, p
    while n:
        if n & 1: res = affine_add(res, pw)
        pw = affine_add(pw, pw)
        n >>= 1
    return res


def _ext(p): return (p[0], p[1], 1, p[0] * p[1] % Q)
def _eadd(p, q):
    A = (p[1] - p[0]) * (q[1] - q[0]) % Q; Bb = (p[1] + p[0]) * (q[1] + q[0]) % Q
    C = 2 * D * p[3] * q[3] % Q; Dd = 2 * p[2] * q[2] % Q
    E, F, G, Hh = Bb - A, Dd - C, Dd + C, Bb + A
    return (E * F % Q, G * Hh % Q, F * G % Q, E * Hh % Q)
def _aff(p):
    zi = pow(p[2], Q - 2, Q)
    return (p[0] * zi % Q, p[1] * zi % Q)
def fast_add(p, q): return _aff(_eadd(_ext(p), _ext(q)))
def fast_mul(p, n):
    acc, e = _ext(ZERO), _ext(p)
    for bit in bin(n)[2:] if n else "":
        acc = _eadd(acc, acc)
        if bit == "1": acc = _eadd(acc, e)
    return _aff(acc)


def _ops(chain): return (chain_mul, affine_add) if chain else (fast_mul, fast_add)
def gen_s(digest32):                                          # ed25519_sha512.rs:100-113
    b = bytearray(digest32)
    b[31] &= 0x7F; b[31] |= 0x40; b[0] &= 0xF8
    return int.from_bytes(b, "little")


def pub_from_scalar(s, chain=False):
    """encode(B * base_field().elem(s)) (:121-123): the multiplier is s mod q"""
    return encode_point(_ops(chain)[0](B, s % Q))
def gen_pub_key(prv, chain=False):                            # :115-125
    return pub_from_scalar(gen_s(H(prv)[:32]), chain)


def sign(msg, prv, chain=False):                              # :127-158
    mul = _ops(chain)[0]
    d = H(prv)
    s, prefix = gen_s(d[:32]), d[32:]
    A = encode_point(mul(B, s % Q))
    r = int.from_bytes(H(prefix + bytes(msg)), "little") % L
    R = encode_point(mul(B, r % Q))
    k = int.from_bytes(H(R + A + bytes(msg)), "little") % L
    return R + ((r + k * s) % L).to_bytes(32, "little")


def verify(sig, pub, msg, chain=None):                        # :160-186
    """chain=None: the chain exactly where a decoded point is off the curve"""
    S = int.from_bytes(sig[32:], "little")
    if S >= L: return False
    Rp = decode_point(sig[:32])
    R = encode_point(Rp)
    k = int.from_bytes(H(R + bytes(pub) + bytes(msg)), "little")
    Ap = decode_point(pub)
    if chain is None: chain = not (on_curve(Rp) and on_curve(Ap))
    mul, add = _ops(chain)
    lhs = mul(B, (S * 8) % L)
    rhs = add(mul(Rp, 8 % L), mul(Ap, (k * 8) % L))
    return lhs == rhs


# ---- helpers for the case lists ---------------------------------------------------------------------------------------------------------------
class _Rng:
    def __init__(self, seed): self.k, self.i = seed, 0
    def bytes(self, n):
        out = b""
        while len(out) < n:
            out += hashlib.sha256(b"ed25519-model %d %d" % (self.k, self.i)).digest(); self.i += 1
        return out[:n]
    def below(self, m): return int.from_bytes(self.bytes(40), "little") % m


def torsion8():
    """a point of order exactly 8"""
    y = 2
    while True:
        p = (recover_x(y, 0), y)
        if on_curve(p):
            t = fast_mul(p, L)
            if fast_mul(t, 4) != ZERO: return t
        y += 1


def off_curve_encodings(rng, n):
    out = []
    while len(out) < n:
        b = rng.bytes(32)
        if not on_curve(decode_point(b)): out.append(b)
    return out


def sign_with_scalar(a, A_bytes, msg, r, R_point=None):
    """a signature under the public key bytes A (whose B-part is a B) with the nonce r; R_point overrides the point sent (r B by default)"""
    Rp = R_point if R_point is not None else fast_mul(B, r)
    R = encode_point(Rp)
    k = int.from_bytes(H(R + A_bytes + msg), "little") % L
    return R + ((r + k * a) % L).to_bytes(32, "little")


MSG_LENGTHS = (0, 1, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96, 97, 1023)      # the block edges of prefix‖msg and R‖A‖msg


def vectors():
    import json, os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ed25519_kats.json")) as f:
        return [{k: (v if k == "name" else bytes.fromhex(v)) for k, v in e.items()} for e in json.load(f)["vectors"]]


_CACHE = {}


def verify_cases(seed=8032, n_honest=64):
    """[{kind, msg, sig, pub, want}] covering the issue's list; `want` comes from verify() and from nowhere else.  Built once per process."""
    key = ("verify", seed, n_honest)
    if key in _CACHE: return _CACHE[key]
    rng = _Rng(seed)
    cases = []
    def add(kind, msg, sig, pub): cases.append({"kind": kind, "msg": bytes(msg), "sig": bytes(sig), "pub": bytes(pub)})
    for v in vectors(): add("vector " + v["name"], v["msg_hex"], v["sig"], v["pub"])
    honest = []
    for t in range(n_honest):
        prv, msg = rng.bytes(32), rng.bytes(MSG_LENGTHS[t % len(MSG_LENGTHS)] if t % 5 else 64)
        pub, sig = gen_pub_key(prv), None
        sig = sign(msg, prv)
        honest.append((msg, sig, pub)); add("honest", msg, sig, pub)
    def flip(b, bit): b = bytearray(b); b[bit >> 3] ^= 1 << (bit & 7); return bytes(b)
    for t in range(4):
        msg, sig, pub = honest[5 * t + 1]
        add("flip R", msg, flip(sig, (t * 67 + 3) % 256), pub)
        add("flip S", msg, flip(sig, 256 + (t * 59 + 1) % 252), pub)
        add("flip key", msg, sig, flip(pub, (t * 71 + 5) % 256))
        if msg: add("flip message", flip(msg, (t * 13) % (8 * len(msg))), sig, pub)
        add("wrong key", msg, sig, honest[5 * t + 2][2])
        add("wrong message", msg + b"x", sig, pub)
    msg, sig, pub = honest[3]
    Sv = int.from_bytes(sig[32:], "little")
    for name, S in (("S=0", 0), ("S=l-1", L - 1), ("S=l", L), ("S=S+l", Sv + L), ("S=2^256-1", 2 ** 256 - 1)):
        add(name, msg, sig[:32] + S.to_bytes(32, "little"), pub)
    # r = 0: R = (0, 1) sent three ways; k hashes the canonical re-encoding each time, so S = k a does for all three
    a = 1 + rng.below(L - 1); A = encode_point(fast_mul(B, a))
    for name, Rb in (("r=0 canonical", (1).to_bytes(32, "little")), ("r=0 y=q+1", (Q + 1).to_bytes(32, "little")), ("r=0 sign bit on x=0", (1 | (1 << 255)).to_bytes(32, "little"))):
        m = rng.bytes(20)
        s0 = sign_with_scalar(a, A, m, 0, ZERO)
        add(name, m, Rb + s0[32:], A)
    # a small-order key: y = 0, x = +-I (order 4), sent as the bytes of q and as canonical bytes.  S = r signs for it exactly where 8k mod l kills the key.
    for name, Ab in (("order-4 key as bytes of q", Q.to_bytes(32, "little")), ("order-4 key canonical", (0).to_bytes(32, "little"))):
        for t in range(16):
            m = rng.bytes(t + 1); r = 1 + rng.below(L - 1)
            add(name, m, sign_with_scalar(0, Ab, m, r), Ab)
    # a mixed-order key a B + T8 verifies exactly where 8k mod l is a multiple of 8 (one message in eight): a stream of its own, its seed chosen so that
    # both decisions occur among the 16 messages (test_ed25519_model.py asserts it)
    T8 = torsion8()
    mix = _Rng(seed * 1000 + 1)
    a = 1 + mix.below(L - 1)
    Amix = encode_point(fast_add(fast_mul(B, a), T8))
    for t in range(16):
        m = mix.bytes(t + 3); r = 1 + mix.below(L - 1)
        add("mixed-order key", m, sign_with_scalar(a, Amix, m, r), Amix)
    A = encode_point(fast_mul(B, a))
    for t in range(3):
        m = rng.bytes(33 + t); r = 1 + rng.below(L - 1)
        add("mixed-order R", m, sign_with_scalar(a, A, m, r, fast_add(fast_mul(B, r), fast_mul(T8, 1 + 2 * t))), A)
    for t, enc in enumerate(off_curve_encodings(rng, 6)):
        msg, sig, pub = honest[7 + t]
        if t < 3: add("off-curve R", msg, enc + sig[32:], pub)
        else: add("off-curve A", msg, sig, enc)
    for c in cases:
        c["on_curve"] = on_curve(decode_point(c["sig"][:32])) and on_curve(decode_point(c["pub"]))
        c["want"] = verify(c["sig"], c["pub"], c["msg"])
    _CACHE[key] = cases
    return cases


def decode_cases(seed=5, n_random=40):
    """32-byte strings for decode_point: the edges of the issue, the base point, random strings (about half off the curve)"""
    rng = _Rng(seed)
    out = [(Q + 1).to_bytes(32, "little"), Q.to_bytes(32, "little"), (Q | (1 << 255)).to_bytes(32, "little"), (1 | (1 << 255)).to_bytes(32, "little"),
           (1).to_bytes(32, "little"), (0).to_bytes(32, "little"), (1 << 255).to_bytes(32, "little"), (Q - 1).to_bytes(32, "little"),
           ((Q - 1) | (1 << 255)).to_bytes(32, "little"), b"\xff" * 32, (2 ** 255 - 1).to_bytes(32, "little"), encode_point(B),
           encode_point((Q - B[0], B[1])), (2 ** 255 - 20).to_bytes(32, "little"), (2).to_bytes(32, "little")]
    return out + [rng.bytes(32) for _ in range(n_random)]


def decode_want(b):
    p = decode_point(b)
    return p[0], p[1], on_curve(p)


def sign_cases(seed=11, n_random=12):
    """[(prv, msg)]: the vectors, then random keys over the block-edge lengths"""
    rng = _Rng(seed)
    out = [(v["prv"], v["msg_hex"]) for v in vectors()]
    for t in range(n_random): out.append((rng.bytes(32), rng.bytes(MSG_LENGTHS[(t * 4 + 1) % len(MSG_LENGTHS)])))
    return out


def pack_messages(msgs):
    import numpy as np
    off = np.zeros(len(msgs) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    return np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8).copy(), off


def pack_cases(cases):
    """the ABI arrays of a case list: (msgs u8, offsets u64[n+1], sigs (n, 64) u8, pubs (n, 32) u8)"""
    import numpy as np
    buf, off = pack_messages([c["msg"] for c in cases])
    sigs = np.frombuffer(b"".join(c["sig"] for c in cases), dtype=np.uint8).reshape(-1, 64).copy()
    pubs = np.frombuffer(b"".join(c["pub"] for c in cases), dtype=np.uint8).reshape(-1, 32).copy()
    return buf, off, sigs, pubs
