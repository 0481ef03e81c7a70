"""A plain restatement of the multi-rank combine (k_jac_sum_to_affine, zk-toolkit_amd/csrc/zkt_msm.hip) over an abstract group.

TEST INFRASTRUCTURE.  The kernel sums `count` Jacobian partials as one wave: lane t folds partials t, t + 64, ... (site `loop`), then a six-level LDS tree
(sites `level32` .. `level1`) in which lane t < d adds lane t + d's value if t + d < count.  Here a partial is its discrete logarithm c_i modulo the group
order and None is the point at infinity, so the model can say which exit of jac_add (csrc/curve.h) every single addition takes:

    inf+x  x+inf  inf+inf   an operand at infinity (accumulator first, as the kernel calls jac_add(v, operand))
    equal                   the same point, whatever its representation: H == 0 and Rr == 0 -> jac_dbl
    opposite                P and -P: H == 0, Rr != 0 -> jac_inf
    generic                 everything else

CASES is the list tests/test_gpu_combine.py runs on the device for G1, G2 and secp256k1; every case carries the (site, class) cells it claims to reach and
tests/test_combine_model.py proves the claims, and that the cases together cover the table, on the CPU.  A case names its partials by token (below), so the
same list serves every group; logs(group) gives the tokens' discrete logarithms, and the GPU test asks the library for partials with exactly those.
Whoever changes the lane loop, the tree, jac_add's special exits or the slot layout of zkt_comm.cpp is sent here by SOURCE_LINES."""
import os
from zkt_testlib import R, SECP_N, SplitMix64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MSM_SRC = os.path.join(ROOT, "zk-toolkit_amd", "csrc", "zkt_msm.hip")
CURVE_SRC = os.path.join(ROOT, "zk-toolkit_amd", "csrc", "curve.h")
COMM_SRC = os.path.join(ROOT, "zk-toolkit_amd", "csrc", "zkt_comm.cpp")

LANES = 64
LEVELS = (32, 16, 8, 4, 2, 1)
SITES = ("loop",) + tuple(f"level{d}" for d in LEVELS)
CLASSES = ("inf+x", "x+inf", "inf+inf", "equal", "opposite", "generic")
GROUPS = ("g1", "g2", "secp")
ORDER = {"g1": R, "g2": R, "secp": SECP_N}
HDR_WORDS = 2               # zkt_comm.cpp: status word + padding in front of every rank's payload
GENERIC_N = 200             # distinct generic partials a case may name: ("g", 0) .. ("g", 199)

# the lines restated above: (what, file, text that must occur, how often)
SOURCE_LINES = [
    ("lane loop", MSM_SRC, "for (size_t i = t; i < count; i += %d) v = jac_add<F>(v, ldj(parts + i * stride));" % LANES, 1),
    ("tree levels", MSM_SRC, "for (int d = %d; d >= 1; d >>= 1) {" % LEVELS[0], 1),
    # k_join_windows has the same store under a 16-lane tree: the line is pinned together with this kernel's `for`
    ("tree store", MSM_SRC, "for (int d = %d; d >= 1; d >>= 1) {\n    if (t >= d && t < 2 * d) stj(lds + (t - d) * JW, v);\n" % LEVELS[0], 1),
    ("tree guard", MSM_SRC, "if (t < d && (size_t)(t + d) < count) v = jac_add<F>(v, ldj(lds + t * JW));", 1),
    ("jac_add: equal points double", CURVE_SRC, "    if (F::is_zero(Rr)) return jac_dbl(p);\n", 1),
    ("jac_add: opposite points give infinity", CURVE_SRC, "    if (F::is_zero(Rr)) return jac_dbl(p);\n    return jac_inf<F>();\n", 1),
    ("HDR_WORDS", COMM_SRC, "constexpr size_t HDR_WORDS = %d;" % HDR_WORDS, 1),
    ("SLOT_WORDS", COMM_SRC, "constexpr size_t SLOT_WORDS = PAYLOAD_WORDS + HDR_WORDS;", 1),
    ("stride of the MSM combine", COMM_SRC, "return zkt_internal_jac_sum(grp, c.d_recv + HDR_WORDS, (size_t)c.world.load(), w + HDR_WORDS, zkt_internal_stream(), out);", 1),
]


def source_line_counts():
    """[(what, wanted count, found count)] for SOURCE_LINES"""
    text, out = {}, []
    for what, path, line, count in SOURCE_LINES:
        if path not in text:
            with open(path) as f:
                text[path] = f.read()
        out.append((what, count, text[path].count(line)))
    return out


# ---- the kernel over discrete logarithms --------------------------------------------------------------------------------------------------
def classify(p, q, order):
    """the exit jac_add(p, q) takes; p is the accumulator"""
    if q is None:
        return "inf+inf" if p is None else "x+inf"
    if p is None:
        return "inf+x"
    if p == q:
        return "equal"
    if (p + q) % order == 0:
        return "opposite"
    return "generic"


def _add(p, q, order):
    if q is None: return p
    if p is None: return q
    return (p + q) % order or None


class Run:
    """one pass of the kernel: total (None = infinity), additions [(site, class, lane)], loop_guard [(lane, i, i < count)], tree_guard [(d, lane, lane + d < count)]"""
    def __init__(self, parts, order):
        count = len(parts)
        assert count >= 1 and all(c is None or 0 < c < order for c in parts)
        self.additions, self.loop_guard, self.tree_guard = [], [], []
        v = [None] * LANES
        for t in range(LANES):
            i = t
            while True:
                self.loop_guard.append((t, i, i < count))
                if not i < count:
                    break
                self.additions.append(("loop", classify(v[t], parts[i], order), t))
                v[t] = _add(v[t], parts[i], order)
                i += LANES
        for d in LEVELS:
            lds = {t - d: v[t] for t in range(d, 2 * d)}
            for t in range(d):
                self.tree_guard.append((d, t, t + d < count))
                if t + d < count:
                    self.additions.append((f"level{d}", classify(v[t], lds[t], order), t))
                    v[t] = _add(v[t], lds[t], order)
        self.total = v[0]

    def cells(self):
        return {(site, cls) for site, cls, _ in self.additions}


# ---- tokens -------------------------------------------------------------------------------------------------------------------------------
# ("g", i): generic partial i, distinct odd discrete logarithms.  "P", "-P": a point and its negative; "P'": the same point as "P" from another computation
# (other bytes, the cross-multiplied equality of jac_add); "Q": one more generic point; "inf0": the partial of an all-zero scalar vector; "infn": the partial
# of a resident set of no bases.
INF_TOKENS = ("inf0", "infn")
_logs = {}


def logs(group):
    """dict token -> discrete logarithm (None for the two infinities) of a group; ("g", i) for i < GENERIC_N, "P", "P'", "-P", "Q"; all of them distinct and odd
    except where the token says otherwise (a skipped or twice-read partial changes every sum)"""
    if group not in _logs:
        order, rng, seen = ORDER[group], SplitMix64(0xC0B1 + GROUPS.index(group)), set()

        def fresh():
            while True:
                c = rng.below(order) | 1
                if 0 < c < order and c not in seen and order - c not in seen:
                    seen.add(c)
                    return c
        d = {("g", i): fresh() for i in range(GENERIC_N)}
        d["P"] = d["P'"] = fresh()
        d["-P"] = order - d["P"]
        d["Q"] = fresh()
        d["inf0"] = d["infn"] = None
        _logs[group] = d
    return _logs[group]


class Case:
    def __init__(self, name, tokens, claim):
        self.name, self.tokens, self.count, self.claim = name, list(tokens), len(tokens), set(claim)

    def parts(self, group):
        d = logs(group)
        return [d[t] for t in self.tokens]

    def run(self, group="g1"):
        return Run(self.parts(group), ORDER[group])


def census(case, group="g1"):
    """the (site, class) cells the case reaches"""
    return case.run(group).cells()


def check_claim(case, group="g1"):
    """[] if census(case) shows every cell the case claims, else what is missing"""
    cen = census(case, group)
    return [f"{case.name}: claims {cell}, reaches {sorted(c for c in cen if c[0] == cell[0])} at that site" for cell in sorted(case.claim) if cell not in cen]


# ---- the case list ------------------------------------------------------------------------------------------------------------------------
DISTINCT_COUNTS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)
# (a, b, count): everything is infinity except positions a and b, which meet at exactly one addition: in lane a's loop if b = a + 64, else at level b - a.
# The counts are the smallest that reach it; (0, 32) runs at 65 too, where lane 0's second pass reads an infinity after a live partial.
PAIRS = ((0, 64, 65), (0, 32, 33), (0, 16, 17), (0, 8, 9), (0, 4, 5), (0, 2, 3), (0, 1, 2), (63, 127, 128), (31, 63, 64), (0, 32, 65))
VARIANTS = (("same", "P", "equal"), ("prime", "P'", "equal"), ("opposite", "-P", "opposite"))
ALL_INF_COUNTS = (1, 2, 65)
ALL_EQUAL_COUNTS = (8, 64)
REJECTS = ("count0", "null_partials", "null_out")          # zkt_internal_jac_sum: ZKT_ERR_SHAPE, the output untouched


def meeting_site(a, b):
    return "loop" if b - a == LANES else f"level{b - a}"


def third_position(a, b):
    """where the with-Q form of a pair puts Q: in a lane that meets the pair's sum AFTER the pair has met (so the claimed cell stays what it is) — a lane of the
    level below the meeting, or any other lane if they meet in the loop.  None for (0, 1): their addition is the kernel's last."""
    if b - a == LANES:
        return (a + 32) % LANES if a else 1 + 32           # (0, 64): lane 33, which also reads nothing on its second pass; (63, 127): lane 31
    d = b - a
    return None if d == 1 else a - d // 2 if a else d // 2


def _inf(i):
    return INF_TOKENS[i & 1]                                # both constructions of infinity, alternating


def _build():
    cases = []
    for n in DISTINCT_COUNTS:
        claim = {("loop", "inf+x")} | ({("loop", "generic")} if n > LANES else set()) | {(f"level{d}", "generic") for d in LEVELS if d < n}
        cases.append(Case(f"distinct-{n}", [("g", i) for i in range(n)], claim))
    for a, b, count in PAIRS:
        for vname, tok, cls in VARIANTS:
            base = [_inf(i) for i in range(count)]
            base[a], base[b] = "P", tok
            cases.append(Case(f"pair-{a}-{b}-n{count}-{vname}", base, {(meeting_site(a, b), cls)}))
            q = third_position(a, b)
            if q is not None:
                withq = list(base)
                assert q not in (a, b) and q < count
                withq[q] = "Q"
                cases.append(Case(f"pair-{a}-{b}-n{count}-{vname}-q{q}", withq, {(meeting_site(a, b), cls)}))
    for n in ALL_INF_COUNTS:
        claim = {("loop", "inf+inf")} | {(f"level{d}", "inf+inf") for d in LEVELS if d < n}
        cases.append(Case(f"all-inf-{n}", [_inf(i) for i in range(n)], claim))
    for n in ALL_EQUAL_COUNTS:
        cases.append(Case(f"all-equal-{n}", ["P"] * n, {(f"level{d}", "equal") for d in LEVELS if d < n}))
    return cases


CASES = _build()
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)


def union_census(group="g1"):
    out = set()
    for c in CASES:
        out |= census(c, group)
    return out


def guard_sides(count):
    """dict(loop=(bool, bool), tree=(bool, bool)): was index count - 1 admitted and index count refused by the loop condition / by the tree guard of a run of `count`
    partials.  The tree guard compares t + d <= 63 with count, so from 64 partials on it admits every pair and only the loop condition sits on the edge."""
    r = Run([1] * count, 1 << 61)
    return dict(loop=(any(i == count - 1 and ok for _, i, ok in r.loop_guard), any(i == count and not ok for _, i, ok in r.loop_guard)),
                tree=(any(t + d == count - 1 and ok for d, t, ok in r.tree_guard), any(t + d == count and not ok for d, t, ok in r.tree_guard)))


def report(group="g1"):
    """the table the pull request's summary quotes: per site, the classes the cases reach"""
    u = union_census(group)
    lines = [f"{len(CASES)} cases + {len(REJECTS)} refusals"]
    for s in SITES:
        lines.append(f"{s:8s} " + " ".join(c for c in CLASSES if (s, c) in u))
    return "\n".join(lines)


if __name__ == "__main__":
    for g in GROUPS:
        print(g); print(report(g))
