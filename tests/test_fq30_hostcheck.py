"""Fq on 13 x 30-bit lazily reduced limbs (fp.h, W = 30; Fq30C in zkt_constants.h), the layout the G1 MSM object runs on, in the host build of the kernel
headers (libzkt_hostcheck.so, csrc/hostcheck_fq30.h), against python integers.  No GPU.

Values cross as raw limbs, so the operands here are any value < 4p in any limb pattern, and what comes back is checked for its limbs (< 2^30), its size and its
residue.  The column model below recomputes, from the generated constants alone, the worst case of every column of every product scan."""
import ctypes, os, re
import numpy as np
import pytest
from zkt_testlib import ROOT, Q, R, G1_GEN, SplitMix64, ints_to_arr, g1_arr, g1_from_arr, py_g1_add, py_g1_mul

W, N = 30, 13
M = (1 << W) - 1
RR = 1 << (W * N)                        # the Montgomery radix 2^390
RINV = pow(RR, -1, Q)
_u32p = ctypes.POINTER(ctypes.c_uint32)
p32 = lambda a: a.ctypes.data_as(_u32p)


@pytest.fixture(scope="module")
def H():
    so = os.path.join(ROOT, "zk-toolkit_amd", "libzkt_hostcheck.so")
    assert os.path.exists(so), "build first (__graft_entry__.build())"
    lib = ctypes.CDLL(so)
    lib.zkt_hostcheck_fq30_watch.restype = ctypes.c_longlong
    return lib


def limbs(x):
    assert 0 <= x < RR
    return np.array([(x >> (W * i)) & M for i in range(N)], dtype=np.uint32)


def val(a):
    return sum(int(v) << (W * i) for i, v in enumerate(a))


def lazy_ok(a):
    return all(int(v) <= M for v in a) and val(a) < 4 * Q


# the largest value < 4p whose low twelve limbs are all 2^30 - 1
_t = (4 * Q - 1) >> (W * (N - 1))
ALL_ONES = (_t << (W * (N - 1))) | ((1 << (W * (N - 1))) - 1)
if ALL_ONES >= 4 * Q:
    ALL_ONES -= 1 << (W * (N - 1))
BOUNDARY = [0, 1, Q - 1, Q, 2 * Q, 3 * Q, 4 * Q - 1, ALL_ONES]


def test_boundary_operands_are_what_they_claim():
    assert ALL_ONES < 4 * Q and ALL_ONES + (1 << (W * (N - 1))) >= 4 * Q and all(int(v) == M for v in limbs(ALL_ONES)[:N - 1])


def _prod(H, op, a, b, c, d):
    o0, o1 = np.zeros(N, np.uint32), np.zeros(N, np.uint32)
    assert H.zkt_hostcheck_fq30_prod(op, p32(limbs(a)), p32(limbs(b)), p32(limbs(c)), p32(limbs(d)), p32(o0), p32(o1)) == 0
    return o0, o1


def _check_products(H, a, b, c, d):
    """every product form on one operand quadruple: residue, limbs, size, and the paired forms bit-equal to two single calls"""
    mul_ab, _ = _prod(H, 0, a, b, 0, 0); mul_cd, _ = _prod(H, 0, c, d, 0, 0)
    sqr_a, _ = _prod(H, 1, a, 0, 0, 0); sqr_c, _ = _prod(H, 1, c, 0, 0, 0)
    for got, want in ((mul_ab, a * b), (mul_cd, c * d), (sqr_a, a * a), (sqr_c, c * c)):
        assert all(int(v) <= M for v in got) and val(got) % Q == want * RINV % Q, (a, b, c, d)
        assert val(got) * RR < Q * (RR + 16 * Q), (a, b, c, d)                     # < p (1 + 16 p / 2^390)
    ms, _ = _prod(H, 2, a, b, c, d); ma, _ = _prod(H, 3, a, b, c, d)
    for got, want in ((ms, a * b - c * d), (ma, a * b + c * d)):
        assert all(int(v) <= M for v in got) and val(got) % Q == want * RINV % Q, (a, b, c, d)
        assert val(got) * RR < Q * (RR + 48 * Q), (a, b, c, d)                     # a b + c (8p - d) + m p < 48 p^2 + 2^390 p
    for op, want in ((4, (mul_ab, mul_cd)), (6, (mul_ab, mul_cd)), (5, (sqr_a, sqr_c)), (7, (sqr_a, sqr_c))):
        g0, g1 = _prod(H, op, a, b, c, d)
        assert (g0 == want[0]).all() and (g1 == want[1]).all(), (op, a, b, c, d)


def test_products_on_boundary_operands(H):
    """0, 1, p-1, p, 2p, 3p, 4p-1 and the all-ones value, every pair (so the all-ones value meets itself and each of the others), the second product of a call rotated"""
    k = 0
    for a in BOUNDARY:
        for b in BOUNDARY:
            k += 1
            _check_products(H, a, b, BOUNDARY[(k + 3) % len(BOUNDARY)], BOUNDARY[(k * 5 + 1) % len(BOUNDARY)])
    _check_products(H, ALL_ONES, ALL_ONES, ALL_ONES, ALL_ONES)
    _check_products(H, 4 * Q - 1, 4 * Q - 1, 4 * Q - 1, 0)                          # the largest subtrahend spread: c (8p - 0)


def test_products_on_random_lazy_operands(H):
    rng = SplitMix64(3030)
    for _ in range(3000):
        _check_products(H, *(rng.below(4 * Q) for _ in range(4)))


# ---- the column model -------------------------------------------------------------------------------------------------------------------------------
def _constants():
    text = open(os.path.join(ROOT, "zk-toolkit_amd", "csrc", "zkt_constants.h")).read()
    body = text[text.index("struct Fq30C {"):]
    body = body[:body.index("\n};")]
    tab = lambda name: [int(v.rstrip("ul"), 16) for v in re.search(r"\b" + name + r"\(int \w+\) \{ constexpr \w+ t\[\d+\] = \{([^}]*)\}", body).group(1).split(",")]
    return {k: tab(k) for k in ("mod", "subk", "subk3", "comp", "split_mul", "split_sqr", "split_mul2")} | {"QEST_M": int(re.search(r"QEST_M = (\d+)u", body).group(1))}


def _column_terms(kind, k, pl, subk):
    """worst case of every multiply-add of column k in the order fp.h issues them: operand limbs 2^30 - 1, doubled limbs 2 (2^30 - 1), the limbs of p and of the 8p spread exact"""
    lo, hi = (0, k) if k < N else (k - N + 1, N - 1)
    if kind == "mul":
        t = [M * M] * (hi - lo + 1)
    elif kind == "sqr":
        t = [2 * M * M for i in range(lo, hi + 1) if 2 * i < k] + ([M * M] if k % 2 == 0 else [])
    else:
        t = [v for i in range(lo, hi + 1) for v in (M * M, M * subk[k - i])]
    return t + ([M * pl[k - j] for j in range(k)] + [M * pl[0]] if k < N else [M * pl[k - j] for j in range(k - N + 1, N)])


@pytest.mark.parametrize("kind", ["mul", "sqr", "mul2"])
def test_no_column_overflows_and_the_split_list_is_exact(kind):
    """With the generated splits no running sum reaches 2^64; without them exactly the listed columns would.  The carry into a column is the worst case of the one before."""
    c = _constants()
    assert sum(v << (W * i) for i, v in enumerate(c["mod"])) == Q and sum(v << (W * i) for i, v in enumerate(c["subk"])) == 8 * Q
    masks, carry, need = c["split_" + kind], 0, []
    for k in range(2 * N):
        terms = _column_terms(kind, k, c["mod"], c["subk"])
        assert masks[k] >> len(terms) == 0, "a split past the column's last multiply-add"
        if carry + sum(terms) >= 1 << 64:
            need.append(k)
        run, hi = carry, 0
        for t, v in enumerate(terms):
            if (masks[k] >> t) & 1:
                hi += run >> W; run = min(run, M)
            run += v
            assert run < 1 << 64, (kind, k, t)
        carry = (run >> W) + hi
        assert carry < 1 << 36
    assert need == [k for k in range(2 * N) if masks[k]], (kind, need)
    if kind == "mul":
        assert need == [10, 11, 12, 13, 14]


# ---- sums, differences and the reduction passes -------------------------------------------------------------------------------------------------------
def _lin(H, op, a, b=0, c=0):
    o = np.zeros(N, np.uint32)
    r = H.zkt_hostcheck_fq30_lin(op, p32(limbs(a)), p32(limbs(b)), p32(limbs(c)), p32(o))
    return o, r


def test_sums_and_differences_on_boundary_operands_keep_their_limb_ranges(H):
    """add, sub, neg, sub2 on the boundary set: residue, output range, and the extremes of every limb intermediate against the bounds fp.h states"""
    c = _constants()
    watch = lambda ch, what: int(H.zkt_hostcheck_fq30_watch(ch, what))
    for op, arity, f in ((0, 2, lambda a, b, c_: a + b), (1, 2, lambda a, b, c_: a - b), (2, 1, lambda a, b, c_: -a), (3, 3, lambda a, b, c_: a - b - 2 * c_)):
        H.zkt_hostcheck_fq30_watch_reset()
        for a in BOUNDARY:
            for b in (BOUNDARY if arity >= 2 else [0]):
                for c_ in (BOUNDARY if arity == 3 else [0]):
                    o, r = _lin(H, op, a, b, c_)
                    assert r == 0 and lazy_ok(o) and val(o) % Q == f(a, b, c_) % Q, (op, a, b, c_)
        assert watch(0, 1) >= 0
        if op == 0:                                               # fp_add: limbs < 2^31; the reduction's addend v[i] + carry stays a u32
            assert watch(0, 0) < (1 << 31) + 64 and watch(3, 0) < 36
        elif op in (1, 2):                                        # fp_sub / fp_neg: 0 <= a + subk - b <= 2^30 - 1 + max subk < 3 * 2^30
            assert 0 <= watch(2, 1) and watch(2, 0) <= M + max(c["subk"]) < 3 << 30 and watch(0, 0) < (3 << 30) + 64 and watch(3, 0) < 36
        else:                                                     # fp_sub2: 0 <= subk3 - b - 2c <= max subk3 < 2^32, the 64-bit sum < 2^35, its carry < 2^5
            assert 0 <= watch(2, 1) and watch(2, 0) <= max(c["subk3"]) < 1 << 32 and watch(0, 0) < (1 << 30) + 32 and watch(1, 0) < 1 << 35 and watch(3, 0) < 32
    for a in BOUNDARY:                                            # the zero test and equality on every lazy form
        assert _lin(H, 4, a)[1] == (1 if a % Q == 0 else 0)
        for b in BOUNDARY:
            assert _lin(H, 5, a, b)[1] == (1 if (a - b) % Q == 0 else 0)


# the calling forms of the reduction: (name, value cap, largest limb of the input, units a full set of lower limbs spills into the top limb)
def _forms(c):
    return [("add", 8 * Q, 2 * M, 3), ("sub", 12 * Q, M + max(c["subk"]), 4), ("sub2", 20 * Q, M + max(c["subk3"]), 6)]


def test_fq30_lazy_reduce_quotient_estimate(H):
    """q = floor(top * QEST_M / 2^32) for EVERY reachable top limb of every calling form (numpy, exhaustive).  q is a non-decreasing step function of the top limb, so
    `q p <= v` binds at the first top limb of each step and `v - q p < 4p` at the last: both are checked there with python integers, and fp_lazy_reduce /
    fp_lazy_reduce2 are run on inputs with those top limbs and the lower limbs at both extremes."""
    c = _constants()
    S = W * (N - 1)
    assert c["QEST_M"] == (1 << 32) // ((Q >> S) + 1)
    for name, cap, limb_max, spill in _forms(c):
        assert sum(limb_max << (W * i) for i in range(N - 1)) < spill << S      # a full set of lower limbs is below `spill` units of the top limb
        max_top = cap >> S
        firsts, lasts, prev_q, start = [], [], 0, 0
        firsts.append(0)
        for base in range(0, max_top + 1, 1 << 22):
            tops = np.arange(base, min(base + (1 << 22), max_top + 1), dtype=np.uint64)
            q = (tops * np.uint64(c["QEST_M"])) >> np.uint64(32)
            assert int(q[0]) >= prev_q and (np.diff(q.astype(np.int64)) >= 0).all()
            steps = np.nonzero(np.diff(q.astype(np.int64), prepend=prev_q))[0]
            for s in steps:
                assert int(q[s]) == len(firsts), "q moves in steps of one"
                lasts.append(base + int(s) - 1); firsts.append(base + int(s))
            prev_q = int(q[-1])
        lasts.append(max_top)
        assert len(firsts) == len(lasts) == prev_q + 1
        for qv, (first, last) in enumerate(zip(firsts, lasts)):
            assert qv * Q <= first << S                                          # never overshoots: v - q p >= 0
            assert min(((last + spill) << S) - 1, cap - 1) - qv * Q < 4 * Q      # result < 4p
            for top in {first, last}:
                for low in (0, limb_max):
                    v = [low] * (N - 1) + [top]
                    x = sum(t << (W * i) for i, t in enumerate(v))
                    if x >= cap:
                        continue
                    o = np.zeros(N, np.uint32)
                    if name == "sub2":                                           # the 64-bit form: a limb < 2^30 beside a u32
                        xs = np.array([min(t, M) for t in v], dtype=np.uint32); ss = np.array([t - min(t, M) for t in v], dtype=np.uint32)
                        assert H.zkt_hostcheck_fq30_reduce(1, p32(xs), p32(ss), p32(o)) == 0
                    else:
                        assert H.zkt_hostcheck_fq30_reduce(0, p32(np.array(v, dtype=np.uint32)), None, p32(o)) == 0
                    assert lazy_ok(o) and val(o) % Q == x % Q and val(o) == x - qv * Q, (name, top, low)


# ---- word conversions and inversion ---------------------------------------------------------------------------------------------------------------------
def _words(H, op, inp, nout):
    o = np.zeros(nout, np.uint32)
    assert H.zkt_hostcheck_fq30_words(op, p32(inp), p32(o)) == 0
    return o


def _w12(x):
    return np.array([(x >> (32 * i)) & 0xFFFFFFFF for i in range(12)], dtype=np.uint32)


def test_word_conversions_and_inversion(H):
    rng = SplitMix64(4242)
    canon = [0, 1, 2, Q - 1, Q - 2, (Q + 1) // 2, 1 << 380, (1 << 360) - 1, 1 << 360, M, M + 1] + [rng.below(Q) for _ in range(200)]
    for x in canon:
        raw = _words(H, 0, _w12(x), N)
        assert lazy_ok(raw) and val(raw) % Q == x * RR % Q and val(raw) * RR < Q * (RR + 16 * Q)
        assert sum(int(v) << (32 * i) for i, v in enumerate(_words(H, 1, raw, 12))) == x
    for x in (0, Q - 1):                                             # every lazy representative of 0 and of p - 1 leaves as the canonical residue
        for j in range(4):
            v = x * RR % Q + j * Q
            assert v < 4 * Q
            assert sum(int(t) << (32 * i) for i, t in enumerate(_words(H, 1, limbs(v), 12))) == x, (x, j)
    for x in [1, 2, Q - 1, Q - 2, (Q + 1) // 2, 1 << 31, (1 << 64) + 1] + [rng.below(Q - 1) + 1 for _ in range(300)]:
        for j in (0, 3):
            o = _words(H, 2, limbs(x * RR % Q + j * Q), N)
            assert lazy_ok(o) and val(o) * RINV % Q == pow(x, -1, Q), (x, j)


# ---- the mixed addition -----------------------------------------------------------------------------------------------------------------------------------
def _neg(p):
    return (p[0], -p[1] % Q)


def _acc(H, mode, p, q, signs, lam):
    o = np.zeros((1, 13), np.uint64)
    r = H.zkt_hostcheck_fq30_g1_acc(mode, p32(g1_arr([p])), p32(g1_arr([q])), signs, p32(ints_to_arr([lam], 6)), p32(o))
    assert r == 0, ("the paired and the unpaired sequence differ in a limb" if r == 1 else "bad call", mode, signs, lam)
    return g1_from_arr(o)[0]


@pytest.mark.parametrize("mode", [1, 2], ids=["scaled_accumulator", "from_empty"])
def test_xyzz_add_aff_against_the_affine_group_law(H, mode):
    """generic sums, the accumulator at infinity (mode 2 starts from it), P + P (the doubling exit) and P + (-P), under all four sign combinations; mode 1 carries
    ZZ = lambda^2 != 1.  The unpaired sequence, the paired one with two calls per pair and the paired one with the interleaved scans must agree in every limb.
    y = 0 cannot occur: such a point has order two, and #E(Fq) = h r with h = 0x396C8C005555E1568C00AAAB0000AAAB and r both odd, so E(Fq) has none; the case is skipped."""
    rng = SplitMix64(99)
    P, S = py_g1_mul(G1_GEN, 0x1234567), py_g1_mul(G1_GEN, R - 5)
    pts = [(P, S), (S, P), (P, P), (P, _neg(P)), (_neg(S), S)] + [(py_g1_mul(G1_GEN, rng.below(R)), py_g1_mul(G1_GEN, rng.below(R))) for _ in range(5)]
    for p, q in pts:
        for signs in range(4):
            for lam in (1, 7, Q - 3):
                want = py_g1_add(_neg(p) if signs & 1 else p, _neg(q) if signs & 2 else q)
                assert _acc(H, mode, p, q, signs, lam) == want, (mode, p == q, signs, lam)
