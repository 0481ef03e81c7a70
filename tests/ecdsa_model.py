"""secp256k1 ECDSA over python integers and hashlib: the checker of the ECDSA tests.  verify() and sign() restate
src/building_block/curves/secp256k1/ecdsa.rs line by line (the cited lines); verify_cases() builds the case list the host-check and GPU tests share.

A public key is None (the point at infinity) or a pair of integers (x, y) AS STORED in the ABI struct: verify() reduces both mod p first, which is what the
ABI's loader does with every sp element (PrimeFieldElem::new, prime_field_elem.rs:263-272) and therefore what zkt_secp_is_on_curve_batch sees."""
import hashlib
from zkt_testlib import SECP_P as P, SECP_N as N, SECP_GEN as G, py_secp_add, SplitMix64

RETRY = "retry"


# ---- group arithmetic: Jacobian double-and-add (the affine py_secp_mul of zkt_testlib inverts at every step; the result is the same point) ----
def _jdbl(p):
    X, Y, Z = p
    if Z == 0 or Y == 0: return (1, 1, 0)
    A, B = X * X % P, Y * Y % P
    C = B * B % P
    D = 2 * ((X + B) ** 2 - A - C) % P
    E = 3 * A % P
    X3 = (E * E - 2 * D) % P
    return (X3, (E * (D - X3) - 8 * C) % P, 2 * Y * Z % P)


def _jadd_aff(p, q):
    X, Y, Z = p
    if Z == 0: return (q[0], q[1], 1)
    ZZ = Z * Z % P
    H, Rr = (q[0] * ZZ - X) % P, (q[1] * ZZ * Z - Y) % P
    if H == 0: return _jdbl((q[0], q[1], 1)) if Rr == 0 else (1, 1, 0)
    HH = H * H % P; HHH = H * HH % P; V = X * HH % P
    X3 = (Rr * Rr - HHH - 2 * V) % P
    return (X3, (Rr * (V - X3) - Y * HHH) % P, Z * H % P)


def mul(pt, k):
    """k * pt for an affine point (or None) and an integer k >= 0"""
    if pt is None or k == 0: return None
    acc = (1, 1, 0)
    for b in bin(k)[2:]:
        acc = _jdbl(acc)
        if b == "1": acc = _jadd_aff(acc, pt)
    if acc[2] == 0: return None
    zi = pow(acc[2], -1, P)
    return (acc[0] * zi * zi % P, acc[1] * zi * zi * zi % P)


def neg(pt): return None if pt is None else (pt[0], (-pt[1]) % P)
def on_curve(x, y): return (y * y - x * x * x - 7) % P == 0
def digest(msg): return hashlib.sha256(bytes(msg)).digest()


def lift_x(x, odd=0):
    """the point (x, y) with y of the given parity, or None when x^3 + 7 is no square (p = 3 mod 4)"""
    y2 = (x * x * x + 7) % P
    y = pow(y2, (P + 1) // 4, P)
    if y * y % P != y2: return None
    return (x, y if (y & 1) == odd else P - y)


# ---- ecdsa.rs ----
def gen_pub_key(d):
    return mul(G, d % N)                                         # :33-35


def sign(z_bytes, d, k):
    """ecdsa.rs:49-84 with the nonce given: (r, s), or RETRY where the loop would `continue`.  d, k: any integers, reduced mod n as PrimeFieldElem::new does."""
    d, k = d % N, k % N
    z = int.from_bytes(z_bytes, "big")                           # :55
    p = mul(G, k)                                                # :58
    if p is None: return RETRY                                   # :61
    r = p[0] % N                                                 # :64
    if r == 0: return RETRY                                      # :67
    s = pow(k, -1, N) * (d * r + z % N) % N                      # :71-74
    if s == 0: return RETRY                                      # :77
    return (r, s)                                                # :81


def verify(z_bytes, r, s, Q):
    """ecdsa.rs:88-135.  r, s: integers as given, NOT reduced."""
    if Q is None: return False                                   # :94
    x, y = Q[0] % P, Q[1] % P                                    # the loader's reduction (module docstring)
    if not on_curve(x, y): return False                          # :98
    # :102 n * pub_key == infinity holds for every point of this cofactor-1 curve; test_ecdsa_model.py checks it on the case list
    if r == 0 or s == 0 or N <= r or N <= s: return False        # :105-112
    z = int.from_bytes(z_bytes, "big") % N                       # :116-117
    w = pow(s, -1, N)                                            # :118
    u1, u2 = z * w % N, r * w % N                                # :119-120
    p3 = py_secp_add(mul(G, u1), mul((x, y), u2))                # :124-126
    if p3 is None: return False                                  # :129
    return r == p3[0] % N                                        # :131


# ---- the case list -----------------------------------------------------------------------------------------------------------------------------------
def _b32(v): return int(v).to_bytes(32, "big")


def wrap_points():
    """[(c, R_big, R_small)]: R_big = (n + c, y) and R_small = (c, y') on the curve.  First c = 2, where the issue's wrap point (n + 2, y) lies on the curve
    (asserted here); if x = 2 itself is not on the curve that entry's R_small is None and a second entry holds the nearest small c with BOTH twins on the curve."""
    big = lift_x(N + 2)
    assert big is not None and on_curve(*big) and N + 2 < P
    out = [(2, big, lift_x(2))]
    if out[0][2] is None:
        c = next(c for c in range(3, 1000) if lift_x(c) is not None and lift_x(N + c) is not None)
        out.append((c, lift_x(N + c), lift_x(c)))
    return out


def verify_cases(seed=2024, n_random=6):
    """list of dicts {kind, z (32 bytes), r, s, Q} covering the issue's list; expected decisions come from verify()"""
    rng = SplitMix64(seed)
    cases = []
    def add(kind, z, r, s, Q): cases.append({"kind": kind, "z": bytes(z), "r": int(r), "s": int(s), "Q": Q})
    def signed(d, z, k=None):
        while True:
            kk = k if k is not None else 1 + rng.below(N - 1)
            sg = sign(z, d, kk)
            if sg != RETRY: return sg
            k = None
    msg3, msg4 = digest([1, 2, 3]), digest([1, 2, 3, 4])
    # ecdsa.rs:259-274: private key 1234 over [1, 2, 3]
    r, s = signed(1234, msg3); add("valid d=1234 [1,2,3]", msg3, r, s, gen_pub_key(1234))
    for t in range(n_random):
        d = 1 + rng.below(N - 1); z = _b32(rng.below(1 << 256)); Q = gen_pub_key(d)
        r, s = signed(d, z)
        add("valid", z, r, s, Q)
        add("flip r", z, r ^ (1 << (t * 37 % 256)), s, Q)
        add("flip s", z, r, s ^ (1 << (t * 53 % 256)), Q)
        zz = bytearray(z); zz[t * 5 % 32] ^= 1 << (t % 8); add("flip digest", zz, r, s, Q)
        add("flip Q.x", z, r, s, (Q[0] ^ (1 << (t * 41 % 256)), Q[1]))
        add("other key", z, r, s, gen_pub_key(1 + rng.below(N - 1)))                           # :276-295
        add("other message", msg4 if t == 0 else _b32(rng.below(1 << 256)), r, s, Q)           # :297-317
        for v in (0, N, N + 1, (1 << 256) - 1):                                                # :194-256 and beyond
            add(f"r={v:#x}"[:12], z, v, s, Q); add(f"s={v:#x}"[:12], z, r, v, Q)
        add("Q at infinity", z, r, s, None)                                                    # :176-192
        add("Q=(x,x)", z, r, s, (Q[0], Q[0]))                                                  # :142-174
        add("Q.x=2^256-1", z, r, s, ((1 << 256) - 1, Q[1]))
    # a coordinate >= p: only x < 2^256 - p (about 2^32) leaves room for x + p in 256 bits, and no private key is known for such a point.  A signature that is
    # valid for a GIVEN key needs none: R = a G + b Q, r = x(R) mod n, s = r / b, z = a s.  Stored as (x + p, y) the key is the same point after the loader's reduction.
    Qs = next(pt for pt in (lift_x(x) for x in range(1, 2000)) if pt is not None)
    a_, b_ = 1 + rng.below(N - 1), 1 + rng.below(N - 1)
    R = py_secp_add(mul(G, a_), mul(Qs, b_)); r = R[0] % N; s = r * pow(b_, -1, N) % N; zb = _b32(a_ * s % N)
    add("valid, known-x key", zb, r, s, Qs)
    add("valid, Q.x + p stored", zb, r, s, (Qs[0] + P, Qs[1]))
    add("invalid, Q.x + p stored", zb, r, s ^ 1, (Qs[0] + P, Qs[1]))
    add("Q.y + p: above 2^256, not storable; y = p stored (y = 0 after reduction)", zb, r, s, (Qs[0], P))
    # chosen keys: Q in {G, -G, 2G, 3G, (n-1)G, (n-2)G}, valid and invalid
    for d in (1, N - 1, 2, 3, N - 2):
        Q = gen_pub_key(d); z = _b32(rng.below(1 << 256)); r, s = signed(d, z)
        add(f"valid d={d if d < 10 else 'n-' + str(N - d)}", z, r, s, Q)
        add(f"invalid d={d if d < 10 else 'n-' + str(N - d)}", z, r, (s + 1) % N or 1, Q)
    add("valid Q=-G", msg3, *signed(N - 1, msg3), neg(G))
    # digests at the edges of the reduction
    for zi in (0, N - 1, N, N + 1, (1 << 256) - 1):
        d = 1 + rng.below(N - 1); r, s = signed(d, _b32(zi))
        add(f"valid digest {zi:#x}"[:24], _b32(zi), r, s, gen_pub_key(d))
        add(f"digest {zi:#x} + n"[:24], _b32((zi + N) % (1 << 256)), r, s, gen_pub_key(d))   # the same z mod n where zi + n < 2^256: still valid then
    # the doubling branch: R = 2t G, r = x(R) mod n, s = z / t, d = z / r  =>  u1 G = u2 Q = t G, the last addition doubles: VALID
    # the cancellation branch: d = -z / r  =>  u2 Q = -t G, the sum is the point at infinity: REJECT
    for t in (5, 1 + rng.below(N - 1), N - 3):
        zb = _b32(1 + rng.below(N - 1)); z = int.from_bytes(zb, "big") % N
        R = mul(G, 2 * t % N); r = R[0] % N
        s = z * pow(t, -1, N) % N; d = z * pow(r, -1, N) % N
        add("doubling", zb, r, s, gen_pub_key(d))
        add("cancellation", zb, r, s, gen_pub_key((-d) % N))
    # the wrap branch: R = (n + c, y) on the curve, r = c, any s; Q = (s / r) (R - (z / s) G)  =>  u1 G + u2 Q = R, x(R) mod n = c = r: VALID, yet X != r Z^2
    # the mirror: the same r, s with Q built from the point whose x is c itself
    for c, R_big, R_small in wrap_points():
        for R, kind in ((R_big, f"wrap x=n+{c}"), (R_small, f"wrap mirror x={c}")):
            if R is None: continue
            for s in (1, 1 + rng.below(N - 1)):
                zb = _b32(rng.below(1 << 256)); z = int.from_bytes(zb, "big") % N
                Q = mul(py_secp_add(R, neg(mul(G, z * pow(s, -1, N) % N))), s * pow(c, -1, N) % N)
                add(kind, zb, c, s, Q)
                add(kind + " r+1", zb, c + 1, s, Q)
    return cases


def pack_cases(cases):
    """the ABI arrays of a case list: digests (n, 32) u8, sigs (n, 8) u64 {r, s}, pks (n, 9) u64 {x, y, is_infinity}"""
    import numpy as np
    from zkt_testlib import int_to_limbs
    n = len(cases)
    dig = np.zeros((n, 32), dtype=np.uint8); sigs = np.zeros((n, 8), dtype=np.uint64); pks = np.zeros((n, 9), dtype=np.uint64)
    for i, c in enumerate(cases):
        dig[i] = np.frombuffer(c["z"], dtype=np.uint8)
        sigs[i, :4] = int_to_limbs(c["r"], 4); sigs[i, 4:] = int_to_limbs(c["s"], 4)
        if c["Q"] is None: pks[i, 8] = 1
        else: pks[i, :4] = int_to_limbs(c["Q"][0], 4); pks[i, 4:8] = int_to_limbs(c["Q"][1], 4)
    return dig, sigs, pks


def sign_cases(seed=77):
    """[(z bytes, d, k)] for the signing tests: the edges of the reductions and every reachable retry branch.  (The r == 0 branch, ecdsa.rs:67, needs
    k G = (n, y) — x = n is on the curve or not, but no k is known for it — and cannot be reached by a test.)"""
    rng = SplitMix64(seed)
    out = []
    rnd = lambda: 1 + rng.below(N - 1)
    for d in (0, 1, N - 1, N, (1 << 256) - 1): out.append((_b32(rng.below(1 << 256)), d, rnd()))          # d reduced on load
    for k in (0, N): out.append((_b32(rng.below(1 << 256)), rnd(), k))                                    # k = 0 mod n: retry (:61)
    for k in (N + 5, (1 << 256) - 1): out.append((_b32(rng.below(1 << 256)), rnd(), k))                    # k reduced on load
    for _ in range(2):                                                                                    # s == 0: d = -z / r for that k's r (:77)
        zb, k = _b32(rng.below(1 << 256)), rnd()
        r = mul(G, k)[0] % N
        out.append((zb, (-(int.from_bytes(zb, "big") % N) * pow(r, -1, N)) % N, k))
    for zi in (0, N - 1, N, N + 1, (1 << 256) - 1): out.append((_b32(zi), rnd(), rnd()))                  # digests at the edges of the reduction
    return out
