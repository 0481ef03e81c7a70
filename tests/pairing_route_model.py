"""TEST INFRASTRUCTURE — python-integer model of the pairing entry points: which kernels a call takes, and what it must return.

Routes.  Each pairing entry point picks a batch route by size (launch_tate, zkt_tate.hip; launch_pairing_product_check, zkt_pairing.hip;
zkt_groth16_verify_batch, zkt_groth16.hip), then every element takes one pass: the fast loop (127 steps for a Tate value, 63 for a decision),
the 255-step loop (OK_REDO / TATE_MARK_LONG: Q on the twist outside G2), the reference's own chain (OK_EXACT / TATE_MARK_EXACT: P outside G1 or a point
off its curve), a panic (an argument at infinity, or a multiple of P met by the reference's chain), or, in fail-closed mode, a rejection of what would
have gone to the reference's chain.  `ROUTES` lists every (entry point, batch route, element pass) cell that can occur.

Values.  Points are built from known discrete logarithms wherever they lie in their groups, so an honest Tate value is T^(a b mod r) with
T = tate(G1, G2), and an honest decision is a congruence mod r.  Every other pairing is the reference's chain restated here in python
(pairing.rs:20-100, rational_function.rs:11-102): the Miller loop over the bits of r - 1 with f <- f^2 num / den and f <- f num / den, then the plain
exponent (q^12 - 1) / r.  Only the Fq / Fq2 / Fq12 arithmetic of oracle/fast_model.py is used, none of its fast algorithms.  No oracle, no HIP."""
import os, re, sys
import numpy as np
from zkt_testlib import (Q, R, ROOT, G1_GEN, G2_GEN, G1W, G2W, FQ12, SplitMix64, int_to_limbs, py_g1_add, py_g1_mul, py_g2_add, py_g2_mul,
                         py_twist_point, to_abi_g2, g1_arr, g2_arr, degenerate_g1_points)

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import fast_model as fm                                             # Fq2 / Fq6 / Fq12 arithmetic only

# ---- the switch-over limits (zkt_tate.hip launch_tate: ZKT_DTATE_MAX; zkt_pairing.hip dproduct_limit: ZKT_DPRODUCT_MAX) ----
DTATE_MAX = 24576
DPRODUCT_MAX = 24576


def library_limits():
    """the defaults the library source gives the two switch-over limits: {env name: value}"""
    src = os.path.join(ROOT, "zk-toolkit_amd", "csrc")
    out = {}
    for name, fn in (("ZKT_DTATE_MAX", "zkt_tate.hip"), ("ZKT_DPRODUCT_MAX", "zkt_pairing.hip")):
        with open(os.path.join(src, fn)) as f:
            text = f.read()
        m = re.findall(r'getenv\("' + name + r'"\);\s*return e \? \(size_t\)strtoull\(e, nullptr, 10\) : \(size_t\)(\d+);', text)
        assert len(m) == 1, (fn, name, m)
        out[name] = int(m[0])
    return out


# ---- GT arithmetic --------------------------------------------------------------------------------------------------------
F12_ONE = fm.F12_1
F12_ZERO = (fm.F6_0, fm.F6_0)
FINAL_EXP = (Q ** 12 - 1) // R
L_BITS = [int(c) for c in bin(R - 1)[3:]]                          # pairing.rs:58-73: r - 1, most significant first, leading 1 dropped


def gt_words(a):
    """Fq12 -> the 72 u64 of the ABI layout (the reference's to_strs order, fq12.rs:179-195)"""
    return np.array([w for c in fm.to_ref_order(a) for w in int_to_limbs(c, 6)], dtype=np.uint64)


def _fq12_const(c):
    return (((c[0] % Q, c[1] % Q), fm.F2_0, fm.F2_0), fm.F6_0)


def _embed_g2(qc):
    """g12_point.rs:47-63: (x, y) of E'(Fq2) -> (x / v, y / (v w)) in Fq12 (Fq12::new(w1, w0), Fq6::new(v2, v1, v0))"""
    v = ((fm.F2_0, fm.F2_1, fm.F2_0), fm.F6_0)
    vw = (fm.F6_0, (fm.F2_0, fm.F2_1, fm.F2_0))
    return fm.f12_mul(_fq12_const(qc[0]), fm.f12_inv(v)), fm.f12_mul(_fq12_const(qc[1]), fm.f12_inv(vw))


def _f12_scale(a, s):
    return tuple(tuple(fm.f2_muls(c, s % Q) for c in six) for six in a)


def _f12_add_const(a, s):
    (c0, c1, c2), b = a
    return (((c0[0] + s) % Q, c0[1]), c1, c2), b


def _f12_sub(a, b):
    return tuple(tuple(fm.f2_sub(x, y) for x, y in zip(s, t)) for s, t in zip(a, b))


class ChainPanic(Exception):
    """the reference panics: a multiple of P met by its chain is infinity (rational_function.rs:36)"""


def _line(V, W, X, Y):
    """RationalFunction::new_g1(V, W) evaluated at (X, Y) (rational_function.rs:20-102)"""
    if V is None or W is None:
        raise ChainPanic()
    (x1, y1), (x2, y2) = V, W
    if V == W:
        slope = 3 * x1 * x1 * pow(2 * y1, -1, Q) % Q
    elif x1 == x2 and (y1 + y2) % Q == 0:
        return _f12_add_const(X, -x1)                               # vertical: X - x
    else:
        slope = (y2 - y1) * pow(x2 - x1, -1, Q) % Q
    return _f12_add_const(_f12_sub(Y, _f12_scale(X, slope)), slope * x1 - y1)      # -slope X + Y - y + slope x


def _neg(V):
    return None if V is None else (V[0], -V[1] % Q)


def miller_ref(P, qc):
    """Pairing::calc_g1_g2 (pairing.rs:20-52) for P = (x, y) and Q = ((x0, x1), (y0, y1)): f, or ChainPanic.  The numerators and denominators
    are collected apart and divided once at the end: the same element of Fq12 as the reference's step-by-step f * num * den^-1."""
    X, Y = _embed_g2(qc)
    num, den = F12_ONE, F12_ONE
    V = P
    for bit in L_BITS:
        v2 = py_g1_add(V, V)
        num = fm.f12_mul(fm.f12_sqr(num), _line(V, V, X, Y))
        den = fm.f12_mul(fm.f12_sqr(den), _line(v2, _neg(v2), X, Y))
        V = v2
        if bit:
            vp = py_g1_add(V, P)
            num = fm.f12_mul(num, _line(V, P, X, Y))
            den = fm.f12_mul(den, _line(vp, _neg(vp), X, Y))
            V = vp
    assert den != F12_ZERO, "a denominator vanished at Q: not an input this model covers"
    return fm.f12_mul(num, fm.f12_inv(den))


_tate_cache = {}


def tate_ref(P, qc):
    """Pairing::tate (pairing.rs:86-100) by the plain definition: an Fq12 value, or None where the reference panics.  0^e = 0."""
    key = (P, qc)
    if key not in _tate_cache:
        try:
            f = miller_ref(P, qc)
            _tate_cache[key] = F12_ZERO if f == F12_ZERO else fm.f12_pow(f, FINAL_EXP)
        except ChainPanic:
            _tate_cache[key] = None
    return _tate_cache[key]


G2C = to_abi_g2(G2_GEN)                                             # the generator in (c0, c1) order
_T = []
_gt_cache = {}


def T():
    """tate(G1, G2) from the plain definition, computed once"""
    if not _T:
        _T.append(tate_ref(G1_GEN, G2C))
    return _T[0]


def gt(k):
    """T^(k mod r)"""
    k %= R
    if k not in _gt_cache:
        _gt_cache[k] = fm.f12_pow(T(), k)
    return _gt_cache[k]


# ---- arguments with known logs, and the ones outside their groups ---------------------------------------------------------------
class P1:
    """a G1 argument.  kind: 'g1' (point = log * G1), 'out' (on E, outside G1), 'off' (off E), 'inf'"""
    __slots__ = ("point", "log", "kind")

    def __init__(self, point, log, kind):
        self.point, self.log, self.kind = point, log, kind


class P2:
    """a G2 argument.  kind: 'g2' (point = log * G2), 'twist' (log * G2 + a point of order dividing the twist's cofactor: on E', outside G2,
    and its Tate value against G1 is that of log * G2, since such a point lies in r E(Fq12)), 'off' (off E'), 'inf'"""
    __slots__ = ("point", "log", "kind")

    def __init__(self, point, log, kind):
        self.point, self.log, self.kind = point, log, kind


_pt_cache = {}


def _memo(key, fn):
    if key not in _pt_cache:
        _pt_cache[key] = fn()
    return _pt_cache[key]


def g1(a):
    a %= R
    return _memo(("g1", a), lambda: P1(py_g1_mul(G1_GEN, a), a, "g1"))


def g2(b):
    b %= R
    return _memo(("g2", b), lambda: P2(py_g2_mul(G2C, b), b, "g2"))


def g2_cofactor_point():
    """[r] of a generic point of E'(Fq2): order divides the twist's cofactor, not infinity"""
    def make():
        q = py_g2_mul(py_twist_point(SplitMix64(4242)), R)
        assert q is not None
        return q
    return _memo("g2cof", make)


def g2_twist(b):
    """b * G2 + a cofactor-order point: on E', outside G2 (b = 0: the cofactor point alone)"""
    b %= R
    return _memo(("tw", b), lambda: P2(py_g2_add(py_g2_mul(G2C, b) if b else None, g2_cofactor_point()), b, "twist"))


def g2_off(b):
    """b * G2 with y0 + 1: off E'"""
    def make():
        (x, (y0, y1)) = g2(b).point
        return P2((x, ((y0 + 1) % Q, y1)), None, "off")
    return _memo(("g2off", b % R), make)


def _degenerate(label):
    return dict(degenerate_g1_points())[label]


def g1_out(a):
    """a * G1 + a point of large cofactor order: on E, outside G1"""
    a %= R
    return _memo(("out", a), lambda: P1(py_g1_add(py_g1_mul(G1_GEN, a), _degenerate("cofactor subgroup, large order")), None, "out"))


def g1_order3():
    """(0, 2), of order 3: the reference's chain meets infinity at its third multiple"""
    return P1((0, 2), None, "out")


def g1_off(a):
    """a * G1 with y + 1: off E"""
    def make():
        x, y = g1(a).point
        return P1((x, (y + 1) % Q), None, "off")
    return _memo(("g1off", a % R), make)


G1_INF = P1(None, None, "inf")
G2_INF = P2(None, None, "inf")

# ---- element classes ------------------------------------------------------------------------------------------------------------
HONEST, Q_TWIST, Q_OFF, P_OUT_VALUE, P_OUT_PANIC, P_OFF, P_OUT_Q_TWIST, INF = (
    "HONEST", "Q_TWIST", "Q_OFF", "P_OUT_VALUE", "P_OUT_PANIC", "P_OFF", "P_OUT+Q_TWIST", "INF")
CLASSES = (HONEST, Q_TWIST, Q_OFF, P_OUT_VALUE, P_OUT_PANIC, P_OFF, P_OUT_Q_TWIST, INF)


def pair_value(p, q):
    """the reference's tate(P, Q): Fq12, or None (panic).  In-group arguments by bilinearity, everything else by the plain chain."""
    if p.kind == "inf" or q.kind == "inf":
        return None
    if p.kind == "g1" and q.kind in ("g2", "twist"):
        return gt(p.log * q.log)
    return tate_ref(p.point, q.point)


def classify(p, q):
    if p.kind == "inf" or q.kind == "inf":
        return INF
    if p.kind == "g1":
        return {"g2": HONEST, "twist": Q_TWIST, "off": Q_OFF}[q.kind]
    if p.kind == "off":
        return P_OFF
    assert p.kind == "out" and q.kind in ("g2", "twist"), (p.kind, q.kind)
    if q.kind == "twist":
        return P_OUT_Q_TWIST
    return P_OUT_VALUE if tate_ref(p.point, q.point) is not None else P_OUT_PANIC


# ---- passes and routes ----------------------------------------------------------------------------------------------------------
SHORT, ATE, FAST127, LONG, EXACT, LONG_EXACT, EXACT_PANIC, INF_PANIC, FAIL_CLOSED = (
    "short", "ate", "127", "long", "exact", "long->exact", "exact-panic", "inf-panic", "fail-closed")

TATE_ROUTES = ("k_dtate", "k_tate")
PRODUCT_ROUTES = ("k_dproduct_ate", "k_pairing_product_check_ate")
GROTH16_ROUTES = ("small/127", "small/ate", "large/127", "large/ate")
ROUTES = ([("tate", r, p) for r in TATE_ROUTES for p in (SHORT, LONG, EXACT, LONG_EXACT, EXACT_PANIC, INF_PANIC)] +
          [("product", r, p) for r in PRODUCT_ROUTES for p in (ATE, LONG, EXACT, EXACT_PANIC, INF_PANIC, FAIL_CLOSED)] +
          [("bls", r, ATE) for r in PRODUCT_ROUTES] +
          [("groth16", r, p) for r in GROTH16_ROUTES for p in ((ATE if r.endswith("ate") else FAST127), LONG, EXACT, EXACT_PANIC, INF_PANIC, FAIL_CLOSED)])


def tate_route(n):
    return "k_dtate" if n <= DTATE_MAX else "k_tate"


def tate_pass(p, q):
    """launch_tate's passes: tate_short / k_dtate + k_tate_resolve, k_tate_long_marked, k_tate_exact_marked"""
    c = classify(p, q)
    if c == INF:
        return INF_PANIC
    if c == HONEST:
        return SHORT
    if c == Q_TWIST:
        return LONG
    if tate_ref(p.point, q.point) is None:
        return EXACT_PANIC
    return LONG_EXACT if c == P_OUT_Q_TWIST else EXACT


HOSTCHECK_TATE = {SHORT: 0, LONG: 50, EXACT: 100, LONG_EXACT: 100, EXACT_PANIC: 2, INF_PANIC: 2}      # csrc/hostcheck.cpp zkt_hostcheck_tate


def short_loop_guards(p, q):
    """zkt_hostcheck_short_loop_guards bits (1 P on E, 2 r P = infinity, 4 Q in G2, 8 Q on E') and the mask of the bits the model decides"""
    bits = (1 if p.kind in ("g1", "out") else 0) | (2 if p.kind == "g1" else 0) | (4 if q.kind == "g2" else 0) | (8 if q.kind in ("g2", "twist") else 0)
    return bits, (~2 if p.kind == "off" else ~0)                    # r P from the loop on a point off E: not the model's business


def tate_call(pairs):
    """zkt_tate_batch: (status, error index or None, [expected Fq12 or None])"""
    vals, panics = [], []
    for i, (p, q) in enumerate(pairs):
        v = pair_value(p, q)
        if v is None:
            panics.append(i)
        vals.append(v)
    return (2, min(panics), vals) if panics else (0, None, vals)


def product_route(n, K):
    return "k_dproduct_ate" if n * K <= DPRODUCT_MAX else "k_pairing_product_check_ate"


def _exact_or_panic(pairs, fail_closed):
    if fail_closed:
        return FAIL_CLOSED
    return EXACT_PANIC if any(pair_value(p, q) is None for p, q in pairs) else EXACT


def product_pass(pairs, fail_closed=False):
    """launch_pairing_product_check: the 63-step kernels, k_pairing_product_check (OK_REDO), finish_exact (OK_EXACT)"""
    if any(p.kind == "inf" or q.kind == "inf" for p, q in pairs):
        return INF_PANIC
    if all(p.kind == "g1" for p, _ in pairs):
        if all(q.kind == "g2" for _, q in pairs):
            return ATE
        if all(q.kind in ("g2", "twist") for _, q in pairs):
            return LONG
    return _exact_or_panic(pairs, fail_closed)


def _sides_equal(left, right, target=F12_ONE):
    """verifier.rs:36-53 / signature.rs:34-39: lhs == rhs on Fq12, the reference's way"""
    lhs, rhs = F12_ONE, target
    for p, q in left:
        lhs = fm.f12_mul(lhs, pair_value(p, q))
    for p, q in right:
        rhs = fm.f12_mul(rhs, pair_value(p, q))
    return lhs == rhs


def product_ok(pairs, neg, fail_closed=False):
    """expected ok of one element (pass, ok); ok is None for a panic"""
    ps = product_pass(pairs, fail_closed)
    if ps in (INF_PANIC, EXACT_PANIC):
        return ps, None
    if ps == FAIL_CLOSED:
        return ps, 0
    if ps in (ATE, LONG):
        return ps, int(sum((-1 if n else 1) * p.log * q.log for (p, q), n in zip(pairs, neg)) % R == 0)
    return ps, int(_sides_equal([pq for pq, n in zip(pairs, neg) if not n], [pq for pq, n in zip(pairs, neg) if n]))


def product_call(elements, neg, fail_closed=False):
    """zkt_pairing_product_check_batch / zkt_bls_verify_batch: (status, error index or None, passes, [ok])"""
    res = [product_ok(e, neg, fail_closed) for e in elements]
    panics = [i for i, (ps, _) in enumerate(res) if ps in (INF_PANIC, EXACT_PANIC)]
    return (2 if panics else 0), (min(panics) if panics else None), [ps for ps, _ in res], [ok for _, ok in res]


# ---- Groth16 --------------------------------------------------------------------------------------------------------------------
class Key:
    """a verifying key from known logs: alpha, beta (None: the CRS carries null g1_alpha / g2_beta), gamma and delta (P2), kappa = the log of
    the stored gt_alpha_beta (alpha beta for an honest key), u = logs of the statement points"""

    def __init__(self, alpha, beta, gamma, delta, u, kappa=None, null_alpha_beta=False):
        self.alpha, self.beta, self.gamma, self.delta, self.u = alpha, beta, gamma, delta, list(u)
        self.kappa = (alpha * beta % R) if kappa is None else kappa % R
        self.null_alpha_beta = null_alpha_beta

    def servable(self, n_stmt):
        """ate_key_applies and ate_settle_locked (zkt_groth16_vk_cache.cpp): the 63-step route may serve this key"""
        return (1 <= n_stmt <= 12 and not self.null_alpha_beta and self.gamma.kind == "g2" and self.delta.kind == "g2"
                and self.kappa == self.alpha * self.beta % R)


def groth16_route(key, n_stmt, n_proofs, cached):
    """zkt_groth16_verify_batch: cached = the key's entry was built by an earlier call and not evicted since (the large path builds it on the spot)"""
    small = 1 <= n_stmt <= 12 and 3 * n_proofs <= DPRODUCT_MAX
    ate = key.servable(n_stmt) and (cached or not small)
    return ("small/" if small else "large/") + ("ate" if ate else "127")


def groth16_pairs(key, A, B, C, stmt):
    S = sum(s * u for s, u in zip(stmt, key.u)) % R
    return [(A, B), (g1(S) if S else G1_INF, key.gamma), (C, key.delta)]


def groth16_ok(key, route, A, B, C, stmt, fail_closed=False):
    """(pass, ok) of one proof: e(A, B) == alpha_beta e(S, gamma) e(C, delta) (verifier.rs:30-54), ok None for a panic"""
    pairs = groth16_pairs(key, A, B, C, stmt)
    fast = ATE if route.endswith("ate") else FAST127
    ps = product_pass(pairs, fail_closed)
    if ps in (INF_PANIC, EXACT_PANIC):
        return ps, None
    if ps == FAIL_CLOSED:
        return ps, 0
    if ps in (ATE, LONG):
        (a, b), (s, g), (c, d) = [(p.log, q.log) for p, q in pairs]
        return (fast if ps == ATE else LONG), int((a * b - key.kappa - s * g - c * d) % R == 0)
    return ps, int(_sides_equal(pairs[:1], pairs[1:], gt(key.kappa)))


def groth16_call(key, route, proofs, fail_closed=False):
    """proofs: [(A, B, C, stmt)] -> (status, error index or None, passes, [ok])"""
    res = [groth16_ok(key, route, *pf, fail_closed=fail_closed) for pf in proofs]
    panics = [i for i, (ps, _) in enumerate(res) if ps in (INF_PANIC, EXACT_PANIC)]
    return (2 if panics else 0), (min(panics) if panics else None), [ps for ps, _ in res], [ok for _, ok in res]


# ---- ABI arrays ---------------------------------------------------------------------------------------------------------------------
def g1_rows(ps):
    return g1_arr([p.point for p in ps])


def g2_rows(qs):
    return g2_arr([to_abi_g2(q.point) if q.point is not None else None for q in qs])
