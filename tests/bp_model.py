"""TEST INFRASTRUCTURE — Bulletproofs (bulletproofs.rs:19-147) restated over discrete logarithms, python integers only (no GPU, no oracle).

Every generator is k·G for a known k (G = the secp256k1 generator, of prime order SECP_N), so every point the reference forms is
(some integer mod SECP_N)·G, and two points are equal iff their integers are.  `range_proof` and `ipa` follow the reference line by
line on those integers: they give its exact verdict and the discrete logarithms of every point the library reports (out_pts A, S,
T1, T2, P; out_trace L, R, P' per level).  `points` turns the few reported ones into ABI points with python-integer arithmetic.
The vector work is O(n · levels) multiplications mod SECP_N, so the model reaches the sizes the library runs at (2^17)."""
from operator import mul
from types import SimpleNamespace
import numpy as np
from zkt_testlib import SECP_N, SECP_GEN, py_secp_mul, secp_arr, rand_u64_array

N = SECP_N


class Gens:
    """discrete logarithms of the generators: g, h (:59-60), u (:137), gg[n], hh[n]"""

    def __init__(self, g, h, u, gg, hh):
        self.g, self.h, self.u, self.gg, self.hh = g, h, u, list(gg), list(hh)


def dot(a, b):
    return sum(map(mul, a, b)) % N


def pow_seq(b, n):
    """prime_field_elem.rs:346-361: 1, b, b^2, ..., b^(n-1)"""
    out, v = [], 1
    for _ in range(n):
        out.append(v); v = v * b % N
    return out


def points(dlogs):
    """dlogs -> (len, 9) u64 in zkt_secp_affine layout (0 -> the point at infinity)"""
    return secp_arr([py_secp_mul(SECP_GEN, k % N) for k in dlogs])


def ipa(n, gg, hh, u, P, a, b, xs):
    """Bulletproofs::inner_product_argument (:19-55), challenges injected (xs[level], :42).
    Returns (verdict, trace) with trace = [L, R, P'] per level, flat, in the order of out_trace."""
    gg, hh, a, b = list(gg), list(hh), list(a), list(b)
    trace, lv = [], 0
    while n > 1:
        np_ = n // 2
        cL = dot(a[:np_], b[np_:]); cR = dot(a[np_:], b[:np_])                               # :36-37
        L = (dot(gg[np_:], a[:np_]) + dot(hh[:np_], b[np_:]) + u * cL) % N                   # :39
        R = (dot(gg[:np_], a[np_:]) + dot(hh[np_:], b[:np_]) + u * cR) % N                   # :40
        x = xs[lv] % N; xi = pow(x, -1, N)
        gg = [(p * xi + q * x) % N for p, q in zip(gg[:np_], gg[np_:])]                      # :44
        hh = [(p * x + q * xi) % N for p, q in zip(hh[:np_], hh[np_:])]                      # :45
        P = (L * x * x + P + R * xi * xi) % N                                                 # :47
        a = [(p * x + q * xi) % N for p, q in zip(a[:np_], a[np_:])]                         # :49
        b = [(p * xi + q * x) % N for p, q in zip(b[:np_], b[np_:])]                         # :50
        trace += [L, R, P]
        n, lv = np_, lv + 1
    c = a[0] * b[0] % N                                                                       # :28-32
    return P == (gg[0] * a[0] + hh[0] * b[0] + u * c) % N, trace


def _vectors(n, aL, rnd):
    """the vectors and sums of :72-112 that depend only on aL and the draws"""
    alpha, rho, y, z, tau1, tau2, x = rnd[:7]
    sL, sR = rnd[7:7 + n], rnd[7 + n:7 + 2 * n]
    two_n, y_n = pow_seq(2, n), pow_seq(y, n)
    z2 = z * z % N
    aR = [(v - 1) % N for v in aL]                                                            # :75
    l0 = [(v - z) % N for v in aL]                                                            # :88
    r0 = [(yi * (ar + z) + tw * z2) % N for yi, ar, tw in zip(y_n, aR, two_n)]               # :90
    r1 = [yi * s % N for yi, s in zip(y_n, sR)]                                               # :91
    t0, t1, t2 = dot(l0, r0), (dot(sL, r0) + dot(l0, r1)) % N, dot(sL, r1)                   # :93-95
    delta = ((z - z2) * sum(y_n) - z2 * z * sum(two_n)) % N                                  # :112
    return dict(aR=aR, sL=sL, sR=sR, two_n=two_n, y_n=y_n, z2=z2, t0=t0, t1=t1, t2=t2, delta=delta)


def v_star(n, aL, rnd):
    """the committed value v for which (65) holds for this aL and these draws: v = (t0 - delta) / z^2.
    For a bit vector it is <aL, 2^n>; for any other aL it is what V must commit to for the proof to pass (65)."""
    w = _vectors(n, aL, rnd)
    return (w["t0"] - w["delta"]) * pow(w["z2"], -1, N) % N


def range_proof(n, V, aL, gamma, G, rnd, use_ipa, xs=None):
    """Bulletproofs::range_proof (:58-147), every draw injected in the layout of zkto_bp_range_proof / zkt_bp_range_proof:
    rnd = alpha, rho, y, z, tau1, tau2, x, sL[n], sR[n]; G: Gens; V: dlog of the commitment.
    Returns (verdict, [A, S, T1, T2, P]) (dlogs; the library reports these points whatever the verdict)."""
    alpha, rho, y, z, tau1, tau2, x = rnd[:7]
    w = _vectors(n, aL, rnd)
    aR, sL, sR, two_n, y_n, z2, t0, t1, t2 = (w[k] for k in ("aR", "sL", "sR", "two_n", "y_n", "z2", "t0", "t1", "t2"))
    A = (G.h * alpha + dot(G.gg, aL) + dot(G.hh, aR)) % N                                    # :77
    S = (G.h * rho + dot(G.gg, sL) + dot(G.hh, sR)) % N                                      # :82
    T1 = (G.g * t1 + G.h * tau1) % N; T2 = (G.g * t2 + G.h * tau2) % N                       # :99-100
    x2 = x * x % N
    t_hat = (t0 + t1 * x + t2 * x2) % N                                                       # :104
    tau_x = (tau2 * x2 + tau1 * x + z2 * gamma) % N                                           # :105
    mu = (alpha + rho * x) % N                                                                # :106
    hhp = [k * yi % N for k, yi in zip(G.hh, pow_seq(pow(y, -1, N), n))]                      # :109
    lhs65 = (G.g * t_hat + G.h * tau_x) % N                                                   # :114
    rhs65 = (V * z2 + G.g * w["delta"] + T1 * x + T2 * x2) % N                                # :115
    l = [(a - z + s * x) % N for a, s in zip(aL, sL)]                                         # :121
    r = [(yi * (ar + z + s * x) + tw * z2) % N for yi, ar, s, tw in zip(y_n, aR, sR, two_n)] # :122
    P = (A + S * x + dot(G.gg, [-z % N] * n) + dot(hhp, [(yi * z + tw * z2) % N for yi, tw in zip(y_n, two_n)])) % N   # :124-128
    pts = [A, S, T1, T2, P]
    if lhs65 != rhs65:                                                                        # :116-118
        return False, pts
    if use_ipa:
        Pp = (P - G.h * mu + G.u * dot(l, r)) % N                                             # :138
        return ipa(n, G.gg, hhp, G.u, Pp, l, r, xs)[0], pts                                   # :139
    if P != (G.h * mu + dot(G.gg, l) + dot(hhp, r)) % N:                                      # :142-145
        return False, pts
    return t_hat == dot(l, r), pts                                                            # :147-149


# ---- instances shared by the CPU and GPU tests ---------------------------------------------------------------------------------
def ints(a):
    """(cnt, 4) u64 -> python ints"""
    return [int.from_bytes(row.tobytes(), "little") for row in np.ascontiguousarray(a)]


def scalars(seed, cnt):
    """(cnt, 4) u64 of odd values below 2^255 < SECP_N: non-zero, canonical, usable as challenges"""
    s = rand_u64_array(seed, (cnt, 4)); s[:, 3] >>= np.uint64(1); s[:, 0] |= np.uint64(1)
    return s


def levels_of(n):
    return max(n.bit_length() - 1, 1)         # one challenge even at n = 1 (unused there)


# kind -> what the instance is; the reference's verdict follows from the model, EXPECT is what the kind is built to give
KINDS = ("honest", "zero", "max", "v_inf", "y_one", "nonbit", "nonbit_vstar")
EXPECT = {"honest": True, "zero": True, "max": True, "v_inf": True, "y_one": True, "nonbit": False, "nonbit_vstar": True}


def rp_instance(kind, n, seed):
    """One instance of `kind`: arrays for the ABI (aL, gamma, rnd, xs) and the same values as python ints (aLi, gammai, rndi, xsi);
    V(G) is the commitment's dlog over generators G, V = g v + h gamma.  The kinds:
      honest        random bits, V = g v + h gamma (v = <aL, 2^n>)
      zero, max     value 0 (aL all zero), value 2^n - 1 (aL all one)
      v_inf         value 0 and gamma = 0: V is the point at infinity
      y_one         random bits, the challenge y = 1 (y^i = y^-i = 1)
      nonbit        random bits with one entry 2, V = g <aL, 2^n> + h gamma: the reference rejects at (65)
      nonbit_vstar  the same aL, V = g v* + h gamma with v* = (t0 - delta) / z^2: (65) holds and the reference accepts; V is not g <aL,2^n> + h gamma"""
    bits = rand_u64_array(seed, (n,)) & np.uint64(1)
    if kind in ("zero", "v_inf"): bits[:] = 0
    if kind == "max": bits[:] = 1
    if kind.startswith("nonbit"): bits[(n * 3) // 4] = 2
    aL = np.zeros((n, 4), np.uint64); aL[:, 0] = bits
    aLi = [int(v) for v in bits]
    gamma = np.zeros((1, 4), np.uint64) if kind == "v_inf" else scalars(seed + 1, 1)
    gammai = ints(gamma)[0]
    rnd = scalars(seed + 2, 7 + 2 * n)
    if kind == "y_one": rnd[2] = [1, 0, 0, 0]
    rndi = ints(rnd)
    xs = scalars(seed + 3, levels_of(n))
    v = v_star(n, aLi, rndi) if kind == "nonbit_vstar" else dot(aLi, pow_seq(2, n))
    return SimpleNamespace(kind=kind, n=n, aL=aL, aLi=aLi, gamma=gamma, gammai=gammai, rnd=rnd, rndi=rndi, xs=xs, xsi=ints(xs),
                           V=lambda G: (G.g * v + G.h * gammai) % N)


def ipa_instance(n, seed, G):
    """a, b, challenges, and the honest P = g^a h^b u^<a,b> (:17) over generators G as a dlog"""
    a, b, xs = scalars(seed, n), scalars(seed + 1, n), scalars(seed + 2, levels_of(n))
    ai, bi = ints(a), ints(b)
    return SimpleNamespace(n=n, a=a, ai=ai, b=b, bi=bi, xs=xs, xsi=ints(xs), P=(dot(G.gg, ai) + dot(G.hh, bi) + G.u * dot(ai, bi)) % N)
