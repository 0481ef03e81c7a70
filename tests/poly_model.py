"""Dense Fr polynomials in python integers, independent of the HIP path and of the oracle, plus a restatement of the host plan of csrc/zkt_poly.hip.

Arithmetic: `kron_mul` (Kronecker substitution: one big-integer product), `school_mul` and `long_division` (the reference's loops, polynomial.rs:173-238, for
cross-checks below ~128 coefficients), `divrem` (power series recurrence + one product), `tree_t` (product tree for t = prod (x - i)), `horner`.
Plan: which product, division, remainder, tree and evaluation path a call takes and how many k_ntt_group launches a transform is; `census_*` name the cells a
call reaches, `CELLS` lists every cell, and the case lists of tests/test_gpu_poly.py (`mul_shapes()` ...) are derived from the constants the SOURCE holds, so
tests/test_poly_model.py can prove that the GPU cases reach every cell whatever the thresholds are."""
import os, re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "zk-toolkit_amd", "csrc", "zkt_poly.hip")
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001

# ---- the plan's constants, as the model holds them (test_poly_model compares them with the source) -------------------------------
POLY_DIRECT_MAX = 64
POLY_DIV_DIRECT_MAX = 64
POLY_MAX_LEN = 1 << 21
NTT_TILE_LOG = 10               # zkt_fr_vec.hip: the contiguous launch covers up to 10 stages, strided launches up to 8 each
NTT_MAX_STAGES = 8
EVAL_ITEMS, EVAL_TPB = 16, 256
EVAL_CHUNK = EVAL_ITEMS * EVAL_TPB
EVAL_SPLIT_MIN_N = 2 * EVAL_CHUNK
EVAL_SPLIT_MAX_K = 1024


def model_constants():
    return {"POLY_DIRECT_MAX": POLY_DIRECT_MAX, "POLY_DIV_DIRECT_MAX": POLY_DIV_DIRECT_MAX, "POLY_MAX_LEN": POLY_MAX_LEN, "EVAL_ITEMS": EVAL_ITEMS,
            "EVAL_TPB": EVAL_TPB, "EVAL_SPLIT_MIN_N": EVAL_SPLIT_MIN_N, "EVAL_SPLIT_MAX_K": EVAL_SPLIT_MAX_K}


def library_constants():
    """the same constants as the library source and the header write them"""
    with open(SRC) as f:
        text = f.read()
    def one(pattern):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return m[0]
    d = int(one(r"\nstatic constexpr size_t POLY_DIRECT_MAX = (\d+);"))
    dd = int(one(r"\nstatic constexpr size_t POLY_DIV_DIRECT_MAX = (\d+);"))
    items, tpb = one(r"static constexpr int EVAL_ITEMS = (\d+), EVAL_TPB = (\d+), EVAL_CHUNK = EVAL_ITEMS \* EVAL_TPB;")
    min_n = int(one(r"static constexpr size_t EVAL_SPLIT_MIN_N = (\d+) \* \(size_t\)EVAL_CHUNK;"))
    max_k = int(one(r"static constexpr size_t EVAL_SPLIT_MAX_K = (\d+);"))
    one(r"if \(\(na < nb \? na : nb\) <= POLY_DIRECT_MAX\)")            # the product's rule
    one(r"if \(L <= POLY_DIV_DIRECT_MAX\)")                             # the quotient's rule
    one(r"if \(\(L < nb \? L : nb\) <= POLY_DIRECT_MAX\)")              # the remainder's rule
    one(r"if \(sp <= POLY_DIRECT_MAX\)")                                # the tree's rule
    one(r"if \(n >= EVAL_SPLIT_MIN_N && k < EVAL_SPLIT_MAX_K\)")        # the evaluation's rule
    with open(os.path.join(ROOT, "include", "zkt.h")) as f:
        hdr = f.read()
    max_len = re.findall(r"^#define ZKT_POLY_MAX_LEN \(\(size_t\)1 << (\d+)\)", hdr, flags=re.M)
    assert len(max_len) == 1, max_len
    return {"POLY_DIRECT_MAX": d, "POLY_DIV_DIRECT_MAX": dd, "POLY_MAX_LEN": 1 << int(max_len[0]), "EVAL_ITEMS": int(items), "EVAL_TPB": int(tpb),
            "EVAL_SPLIT_MIN_N": min_n * int(items) * int(tpb), "EVAL_SPLIT_MAX_K": max_k}


# ---- arithmetic ------------------------------------------------------------------------------------------------------------
def kron_mul(a, b):
    """a * b mod R, exactly len(a) + len(b) - 1 coefficients (not normalised).  Inputs are reduced mod R first."""
    a = [x % R for x in a]; b = [x % R for x in b]
    slot = 2 * 255 + min(len(a), len(b)).bit_length() + 1
    nbytes = (slot + 7) // 8; slot = nbytes * 8                       # whole bytes: packing and unpacking are byte copies
    pack = lambda p: int.from_bytes(b"".join(x.to_bytes(nbytes, "little") for x in p), "little")
    n = len(a) + len(b) - 1
    raw = (pack(a) * pack(b)).to_bytes(nbytes * (n + 1), "little")
    return [int.from_bytes(raw[i * nbytes:(i + 1) * nbytes], "little") % R for i in range(n)]


def school_mul(a, b):
    """Polynomial::multiply_by (polynomial.rs:173-190)"""
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % R
    return out


def trim(p):
    p = list(p)
    while p and p[-1] % R == 0: p.pop()
    return p


def long_division(a, b):
    """Polynomial::divide_by (polynomial.rs:204-238) on un-normalised a: (q of len(a) - len(b) + 1 coefficients, trimmed remainder)"""
    a = [x % R for x in a]; b = [x % R for x in b]
    assert len(a) >= len(b) and b[-1] != 0
    inv = pow(b[-1], -1, R); L = len(a) - len(b) + 1
    q = [0] * L
    for k in range(L - 1, -1, -1):
        c = a[k + len(b) - 1] * inv % R; q[k] = c
        if c:
            for d, y in enumerate(b): a[k + d] = (a[k + d] - c * y) % R
    return q, trim(a[:len(b) - 1])


def divrem(a, b):
    """the same result by the power series recurrence on the reversed operands (O(L min(L, nb))) and one Kronecker product"""
    a = [x % R for x in a]; b = [x % R for x in b]
    assert len(a) >= len(b) and b[-1] != 0
    na, nb = len(a), len(b); L = na - nb + 1
    inv = pow(b[-1], -1, R)
    f = b[::-1][:L]; rq = []
    for k in range(L):
        acc = a[na - 1 - k]
        for j in range(1, min(k, len(f) - 1) + 1): acc -= f[j] * rq[k - j]
        rq.append(acc % R * inv % R)
    q = rq[::-1]
    qb = kron_mul(q, b)
    return q, trim([(x - y) % R for x, y in zip(a[:nb - 1], qb[:nb - 1])])


def tree_t(n):
    """prod_{i=1..n} (x - i), n + 1 coefficients, by a product tree over kron_mul"""
    level = [[(-i) % R, 1] for i in range(1, n + 1)] or [[1]]
    while len(level) > 1:
        level = [kron_mul(level[i], level[i + 1]) if i + 1 < len(level) else level[i] for i in range(0, len(level), 2)]
    return level[0]


def horner(p, x):
    acc = 0
    for c in reversed(p): acc = (acc * x + c) % R
    return acc


def shifted_sum(terms, b, n):
    """sum of c x^d b(x) over the (d, c) of `terms`, n coefficients: a sparse polynomial times a dense one in O(len(terms) len(b))"""
    out = [0] * n
    for d, c in terms:
        for j, y in enumerate(b): out[d + j] = (out[d + j] + c * y) % R
    return out


# ---- the host plan ---------------------------------------------------------------------------------------------------------
def log2_ceil(x):
    k = 1
    while (1 << k) < x: k += 1
    return k


def ntt_launches(logN):
    """k_ntt_group launches of one transform: 1 for logN <= 10, 2 for 11..18, 3 from 19"""
    rem = logN - min(logN, NTT_TILE_LOG); k = 1
    while rem > 0: rem -= min(rem, NTT_MAX_STAGES); k += 1
    return k


def mul_plan(na, nb, same=False, D=None):
    D = POLY_DIRECT_MAX if D is None else D
    if min(na, nb) <= D: return {"path": "direct"}
    logN = log2_ceil(na + nb - 1)
    return {"path": "ntt", "logN": logN, "launches": ntt_launches(logN), "transforms": 2 if same else 3, "square": same}


def newton_steps(L):
    """transform sizes N = 2p of the Newton steps p -> 2p that take 1 / rev(b) from precision 1 to at least L"""
    out, p = [], 1
    while p < L: out.append(2 * p); p *= 2
    return out


def div_plan(na, nb, D=None, Dd=None):
    D = POLY_DIRECT_MAX if D is None else D; Dd = POLY_DIV_DIRECT_MAX if Dd is None else Dd
    L = na - nb + 1
    plan = {"L": L, "quotient": "direct" if L <= Dd else "newton", "steps": [] if L <= Dd else newton_steps(L)}
    if L > Dd: plan["final"] = "halves" if 2 * L - 1 > POLY_MAX_LEN else "whole"          # rev(a) g mod x^L: one product, or three products of halves
    plan["rem"] = "none" if nb == 1 else "direct" if min(L, nb) <= D else "fold"
    if plan["rem"] == "fold": plan["rem_logN"] = log2_ceil(nb - 1)
    return plan


def tree_levels(n, D=None):
    """levels of the product tree, bottom up: (span of the children, nodes produced, 'direct' | 'ntt', some node has one child only, some node has two full children)"""
    D = POLY_DIRECT_MAX if D is None else D
    out, sp = [], 1
    while sp < n:
        nodes = (n + 2 * sp - 1) // (2 * sp)
        deg = lambda j: max(0, min(sp, n - j * sp))
        only = any(deg(2 * j + 1) == 0 for j in range(max(0, nodes - 2), nodes))
        out.append((sp, nodes, "direct" if sp <= D else "ntt", only, deg(1) == sp))
        sp *= 2
    return out


def eval_plan(n, k):
    return "split" if n >= EVAL_SPLIT_MIN_N and k < EVAL_SPLIT_MAX_K else "horner"


CELLS = ["mul_direct", "mul_direct_edge", "mul_ntt_edge", "mul_ntt_1", "mul_ntt_2", "mul_ntt_3", "mul_square", "mul_max_len",
         "div_direct", "div_direct_edge", "div_newton_edge", "div_newton", "div_newton_ragged", "div_newton_halves", "rem_none", "rem_direct", "rem_fold", "rem_fold_short_divisor",
         "t_empty", "t_leaf", "t_direct", "t_ntt", "t_only_child", "t_wrap",
         "eval_horner", "eval_split", "eval_split_ragged"]


def census_mul(na, nb, same=False, D=None):
    D = POLY_DIRECT_MAX if D is None else D
    p = mul_plan(na, nb, same, D); c = set()
    if p["path"] == "direct":
        c.add("mul_direct")
        if min(na, nb) == D: c.add("mul_direct_edge")
    else:
        c.add("mul_ntt_%d" % p["launches"])
        if min(na, nb) == D + 1: c.add("mul_ntt_edge")
        if same: c.add("mul_square")
    if na + nb - 1 == POLY_MAX_LEN: c.add("mul_max_len")
    return c


def census_div(na, nb, D=None, Dd=None):
    Dd = POLY_DIV_DIRECT_MAX if Dd is None else Dd
    p = div_plan(na, nb, D, Dd); L = p["L"]; c = set()
    if p["quotient"] == "direct":
        c.add("div_direct")
        if L == Dd: c.add("div_direct_edge")
    else:
        c.add("div_newton")
        if L == Dd + 1: c.add("div_newton_edge")
        if L & (L - 1): c.add("div_newton_ragged")
        if p["final"] == "halves": c.add("div_newton_halves")
    c.add("rem_" + p["rem"])
    if p["rem"] == "fold" and nb - 1 < L: c.add("rem_fold_short_divisor")
    return c


def census_t(n, D=None):
    if n == 0: return {"t_empty"}
    if n == 1: return {"t_leaf"}
    c = set()
    for sp, nodes, path, only, full in tree_levels(n, D):
        c.add("t_" + path)
        if only: c.add("t_only_child")
        if path == "ntt" and full: c.add("t_wrap")
    return c


def census_eval(n, k):
    p = eval_plan(n, k)
    return {"eval_" + p} | ({"eval_split_ragged"} if p == "split" and n % EVAL_CHUNK else set())


# ---- the case lists of tests/test_gpu_poly.py, from the constants the source holds ------------------------------------------------
def mul_shapes():
    D = library_constants()["POLY_DIRECT_MAX"]
    return [(1, 1), (1, 5), (5, 1), (D, D), (D + 1, D + 1), (D, 3000), (3000, D + 1), (512, 513), (513, 513), (4096, 4097)]


BIG_MUL = ((1 << 18) + 1, 1 << 18)            # 2^19 coefficients: three launches per transform
LIMIT_MUL = ((1 << 20) + 1, 1 << 20)          # exactly ZKT_POLY_MAX_LEN coefficients


def div_shapes():
    """(L, nb)"""
    Dd = library_constants()["POLY_DIV_DIRECT_MAX"]
    return [(1, 1), (1, 7), (7, 1), (Dd, 33), (Dd + 1, 33), (1000, 1025), (1025, 1000), (4097, 2)]


BIG_DIV = ((1 << 17) + 1, 1 << 17)
LONG_QUOTIENT_DIV = ((1 << 20) + 1, 2)       # 2 L - 1 > ZKT_POLY_MAX_LEN: the last product of the quotient is cut into halves


def t_sizes():
    D = library_constants()["POLY_DIRECT_MAX"]
    return [0, 1, 2, 3, D - 1, D + 1, 1000, 4096]


EVAL_SHAPES = [(1, 1), (2, 64), (1000, 1000), (1 << 20, 1), (1 << 20, 3), (10001, 2)]       # the last: a split whose final block and lane are partly filled
QAP_SIZES = [1, 2, 5, 64, 1000, 1025]


def gpu_case_census():
    """every cell the case lists above reach, with the source's thresholds"""
    k = library_constants(); D, Dd = k["POLY_DIRECT_MAX"], k["POLY_DIV_DIRECT_MAX"]
    c = set()
    for na, nb in mul_shapes() + [BIG_MUL, LIMIT_MUL]: c |= census_mul(na, nb, D=D)
    c |= census_mul(513, 513, same=True, D=D)
    for L, nb in div_shapes() + [BIG_DIV, LONG_QUOTIENT_DIV]: c |= census_div(L + nb - 1, nb, D, Dd)
    for n in t_sizes(): c |= census_t(n, D)
    for n, kk in EVAL_SHAPES: c |= census_eval(n, kk)
    return c
