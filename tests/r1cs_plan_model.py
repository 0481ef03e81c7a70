"""The host plan of the Groth16 R1CS prover (csrc/zkt_groth16_r1cs.hip) restated in python and numpy, with no field arithmetic on the GPU side:
which shard ranges a rank holds, how its quotient convolution is cut into blocks (qcnt, qs0, logM, Bi, M, Q), how every transform of size 2^logN is cut
into k_ntt_group launches (lo, cnt, cbits) and how those launches address their tiles, how many tiles each prefix-product scan needs, which mat-vec rows
go to k_spmv_long, and which stream layout the four resident sums get.  `census(case)` names the cells of this plan that one setup and proof reach;
`CELLS` lists every cell, so tests/test_r1cs_plan_model.py can prove that tests/test_gpu_r1cs_plans.py runs each of them on the GPU."""
import os, re
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "zk-toolkit_amd", "csrc", "zkt_groth16_r1cs.hip")
FR_SRC = os.path.join(ROOT, "zk-toolkit_amd", "csrc", "zkt_fr_vec.hip")      # the transform and the scan

NTT_TILE_LOG = 10           # a k_ntt_group tile holds at most 2^10 elements (32 KB of LDS)
NTT_MAX_STAGES = 8          # stages per strided launch
SMALL_LOGM = 10             # Bi is not cut below min(n, 2^(SMALL_LOGM - 1)) ...: the "logM <= 10" clause
SPMV_LONG = 4096            # rows longer than this go to k_spmv_long
SC_TILE = 256 * 8           # k_scanmul_tile: SC_TPB * SC_ITEMS elements per tile; two levels of tiles
SIDE_BY_SIDE = 1 << 19      # every resident set below this: the four sums on four streams
MAX_N = (SC_TILE * SC_TILE - 1) // 2      # 2n + 1 factorials must fit the two-level scan: n <= 2^21 - 1


def library_constants():
    """the same constants as the library source writes them"""
    with open(FR_SRC) as f:
        text = f.read()
    def one(pattern):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return m[0]
    tile_log = int(one(r"static constexpr int NTT_TILE_LOG = (\d+), NTT_TPB = \d+;"))
    cap = one(r"int cnt = rem < (\d+) \? rem : (\d+), cb = NTT_TILE_LOG - cnt;")
    assert cap[0] == cap[1], cap
    tpb, items = one(r"static constexpr int SC_TPB = (\d+), SC_ITEMS = (\d+), SC_TILE = SC_TPB \* SC_ITEMS;")
    with open(SRC) as f:
        text = f.read()
    clause = int(one(r"\(logM <= (\d+) && \(\(size_t\)1 << \(logM - 1\)\) < n\)"))
    spmv_long = int(one(r"static constexpr uint32_t SPMV_LONG = (\d+);"))
    side = int(one(r"pk->hiC2 - pk->loC2\) < \(\(size_t\)1 << (\d+)\);"))
    one(r"n > ZKT_R1CS_MAX_N")                      # the setup checks the header's limit
    with open(os.path.join(ROOT, "include", "zkt.h")) as f:
        max_n = re.findall(r"^#define ZKT_R1CS_MAX_N (\d+)", f.read(), flags=re.M)
    assert len(max_n) == 1, max_n
    return {"NTT_TILE_LOG": tile_log, "NTT_MAX_STAGES": int(cap[0]), "SMALL_LOGM": clause, "SPMV_LONG": spmv_long,
            "SC_TILE": int(tpb) * int(items), "SIDE_BY_SIDE": 1 << side, "MAX_N": int(max_n[0])}


def model_constants():
    return {"NTT_TILE_LOG": NTT_TILE_LOG, "NTT_MAX_STAGES": NTT_MAX_STAGES, "SMALL_LOGM": SMALL_LOGM, "SPMV_LONG": SPMV_LONG,
            "SC_TILE": SC_TILE, "SIDE_BY_SIDE": SIDE_BY_SIDE, "MAX_N": MAX_N}


# ---- shard ranges and the quotient's block plan ------------------------------------------------------------------------------
def shard_range(tot, shard, nshards):
    base, extra = divmod(tot, nshards)
    lo = shard * base + min(shard, extra)
    return lo, lo + base + (1 if shard < extra else 0)


def _logm(cnt, n, clause=True):
    logM = 1
    while (1 << (logM - 1)) < cnt or (clause and logM <= SMALL_LOGM and (1 << (logM - 1)) < n): logM += 1
    return logM


def block_plan(n, nshards, shard):
    """this rank's range of the n - 1 quotient values and its block sizes: (cnt, s0, Bi, M, Q)"""
    lo, hi = shard_range(n - 1 if n >= 2 else 0, shard, nshards)
    cnt, s0 = hi - lo, lo + 1
    logM = _logm(cnt, n)
    M = 1 << logM; Bi = M // 2; Q = (n + Bi - 1) // Bi if cnt else 1
    return cnt, s0, Bi, M, Q


def plan(n, l, m, shard=0, nshards=1):
    """everything zkt_groth16_setup_r1cs_sharded derives from the sizes alone"""
    nw, nh = m - l, (n - 1 if n >= 2 else 0)
    nA, nC1, nC2 = n + 2, n + nw + 3, nh
    A, C1, C2 = shard_range(nA, shard, nshards), shard_range(nC1, shard, nshards), shard_range(nC2, shard, nshards)
    cnt, s0, Bi, M, Q = block_plan(n, nshards, shard)
    logM = M.bit_length() - 1
    return dict(n=n, l=l, m=m, nw=nw, nh=nh, nA=nA, nC1=nC1, nC2=nC2, A=A, C1=C1, C2=C2, qcnt=cnt, qs0=s0, logM=logM, M=M, Bi=Bi, Q=Q,
                clause_binds=logM != _logm(cnt, n, clause=False), ragged=cnt > 0 and Q > 1 and n % Bi != 0,
                side_by_side=max(A[1] - A[0], C1[1] - C1[0], C2[1] - C2[0]) < SIDE_BY_SIDE)


# ---- the transform: stage groups and k_ntt_group's addressing ----------------------------------------------------------------
def ntt_groups(logN):
    """ntt_groups(): the contiguous group first, then strided groups of <= 8 stages with >= 4 adjacent columns"""
    c0 = min(logN, NTT_TILE_LOG)
    g, lo, rem = [(0, c0, 0)], c0, logN - c0
    while rem > 0:
        cnt = min(rem, NTT_MAX_STAGES); cb = min(NTT_TILE_LOG - cnt, lo)
        g.append((lo, cnt, cb)); lo += cnt; rem -= cnt
    return g


def ntt_launches(p):
    """every k_ntt_group launch of one setup and one proof of plan p, in launch order: (direction, lo, cnt, cbits, grid_x, ny, mulvec).
       Setup transforms the Q kernel slices whatever the rank holds; a proof runs no transform without a quotient value (n = 1, or more ranks than values)."""
    logM, Q = p["logM"], p["Q"]
    g = ntt_groups(logM)
    grid = lambda batch, gr: (batch << logM) >> (gr[1] + gr[2])
    out = [("setup_fwd",) + gr + (grid(Q, gr), 1, False) for gr in reversed(g)]
    if not p["qcnt"]: return out
    out += [("prove_fwd",) + gr + (grid(Q, gr), 3, gr == g[0]) for gr in reversed(g)]
    out += [("prove_inv",) + gr + (grid(1, gr), 3, False) for gr in g]
    return out


def group_tiles(logN, lo, cnt, cbits, batch=1):
    """(blocks, tile) array of the element index g of LDS slot e in block blockIdx.x, exactly as k_ntt_group computes it"""
    tile = 1 << (cnt + cbits); cmask = (1 << cbits) - 1
    bx = np.arange((batch << logN) >> (cnt + cbits), dtype=np.int64)[:, None]
    tph = 1 << (lo - cbits)
    hi, c0 = bx // tph, (bx % tph) << cbits
    e = np.arange(tile, dtype=np.int64)[None, :]
    return (hi << (lo + cnt)) | c0 | ((e >> cbits) << lo) | (e & cmask)


def group_butterflies(logN, lo, cnt, cbits, t, batch=1):
    """local stage t of one launch, every butterfly of every block: (global index of the upper element, of the lower one, twiddle exponent)"""
    cmask = (1 << cbits) - 1
    g = group_tiles(logN, lo, cnt, cbits, batch)
    b = np.arange((1 << (cnt + cbits)) // 2, dtype=np.int64)[None, :]
    cc, kb = b & cmask, b >> cbits
    k0 = ((kb >> t) << (t + 1)) | (kb & ((1 << t) - 1))
    e0 = (k0 << cbits) | cc
    e1 = e0 + (1 << (t + cbits))
    tph = 1 << (lo - cbits)
    c0 = (np.arange(g.shape[0], dtype=np.int64)[:, None] % tph) << cbits
    j = ((k0 & ((1 << t) - 1)) << lo) | c0 | cc
    exp = j << (logN - 1 - lo - t)
    rows = np.arange(g.shape[0])[:, None]
    u, v = g[rows, e0], g[rows, e1]
    return u, v, np.broadcast_to(exp, u.shape)


def textbook_stage(logN, s):
    """radix-2 butterflies of distance 2^s on N = 2^logN points: pairs (i, i + 2^s) for bit s of i clear, twiddle w^((i mod 2^s) 2^(logN-1-s))"""
    i = np.arange(1 << logN, dtype=np.int64)
    i = i[((i >> s) & 1) == 0]
    return i, i + (1 << s), (i & ((1 << s) - 1)) << (logN - 1 - s)


def stage_order(logN, dif):
    """the global stage (butterfly distance 2^s) of every local stage, in execution order: [(group, t, s)]"""
    out = []
    g = ntt_groups(logN)
    for gi in (reversed(range(len(g))) if dif else range(len(g))):
        lo, cnt, _ = g[gi]
        for st in range(cnt):
            t = cnt - 1 - st if dif else st
            out.append((gi, t, lo + t))
    return out


def ntt_through_groups(a, logN, w, R, dif):
    """python-int transform that moves data exactly as the k_ntt_group launches do: DIF natural -> bit-reversed, or DIT bit-reversed -> natural"""
    a = list(a)
    g = ntt_groups(logN)
    tw = [pow(w, k, R) for k in range(max(1, (1 << logN) // 2))]
    for gi, t, s in stage_order(logN, dif):
        lo, cnt, cbits = g[gi]
        u_i, v_i, ex = (x.ravel().tolist() for x in group_butterflies(logN, lo, cnt, cbits, t))
        for i0, i1, e in zip(u_i, v_i, ex):
            u, v = a[i0], a[i1]
            if dif: a[i0], a[i1] = (u + v) % R, (u - v) * tw[e] % R
            else:
                v = v * tw[e] % R
                a[i0], a[i1] = (u + v) % R, (u - v) % R
    return a


def bitrev(k, bits):
    return int(format(k, f"0{bits}b")[::-1], 2) if bits else 0


# ---- prefix-product scans -----------------------------------------------------------------------------------------------
def scan_calls(p):
    """the four scan_mul calls of setup: element counts.  fact: 2n + 1 factorials; pre: prod (x - j), j < 2n; tw, twinv: M/2 powers each"""
    n = p["n"]
    return {"fact": 2 * n + 1, "pre": 2 * n - 1, "tw": p["M"] // 2, "twinv": p["M"] // 2}


def scan_kind(length):
    """one tile / an exact multiple of tiles / a last tile of ONE element / any other ragged last tile; 'limit' past the two levels"""
    tiles = -(-length // SC_TILE)
    if tiles > SC_TILE: return "limit"
    if tiles == 1: return "one_tile"
    if length % SC_TILE == 0: return "exact"
    return "tail1" if length % SC_TILE == 1 else "ragged"


# ---- cells --------------------------------------------------------------------------------------------------------------
MAX_LOGM = 22               # unsharded n = MAX_N: cnt = 2^21 - 2 values, M = 2^22


def _scan_cells():
    cells = set()
    for n in range(1, 1 << 12):           # which kinds each call can reach at all (lengths 2n +- 1 are odd; M/2 is a power of two)
        cells |= {("scan", "fact", scan_kind(2 * n + 1)), ("scan", "pre", scan_kind(2 * n - 1))}
    for logM in range(1, MAX_LOGM + 1):
        cells |= {("scan", k, scan_kind(1 << (logM - 1))) for k in ("tw", "twinv")}
    return cells


def _ntt_cells():
    """a proof transforms at logM >= 2 only: a rank with a quotient value has n >= 2, and the clause keeps Bi >= min(n, 512)"""
    cells = set()
    for logM in range(1, MAX_LOGM + 1):
        for gr in ntt_groups(logM):
            cells |= {("ntt", d) + gr for d in (("setup_fwd", "prove_fwd", "prove_inv") if logM >= 2 else ("setup_fwd",))}
    return cells


CELLS = frozenset(_ntt_cells() | _scan_cells() | {
    ("blocks", "Q>1"), ("blocks", "ragged"), ("blocks", "full_last"), ("blocks", "qcnt0"), ("blocks", "clause_binds"), ("blocks", "ranks_differ_logM"),
    ("spmv", "rowwise", "at_limit"), ("spmv", "rowwise", "long"), ("spmv", "colwise", "long"),
    ("streams", "side_by_side"), ("streams", "shared"),
    ("wires", "nw0"), ("wires", "nh0"), ("wires", "unused_stmt"), ("wires", "unused_wit"), ("wires", "l>1"),
    ("reject", "n_limit"), ("reject", "nshards>n"), ("reject", "x_in_domain")})


def census(case):
    """the cells one case reaches.  case: dict with n, l, m, nshards (default 1), and optionally
       row_max / col_max (longest row of A, B or C and longest wire column), row_lens (every row length that occurs among the long-row candidates),
       unused_stmt / unused_wit (a wire in no constraint), reject ('n_limit' | 'nshards>n' | 'x_in_domain')"""
    if case.get("reject"): return {("reject", case["reject"])}
    n, l, m, W = case["n"], case["l"], case["m"], case.get("nshards", 1)
    out = set()
    plans = [plan(n, l, m, k, W) for k in range(W)]
    for p in plans:
        for d, lo, cnt, cbits, *_ in ntt_launches(p):
            out.add(("ntt", d, lo, cnt, cbits))
        out |= {("scan", k, scan_kind(length)) for k, length in scan_calls(p).items()}
        if not p["qcnt"] and n >= 2: out.add(("blocks", "qcnt0"))
        if p["qcnt"] and p["Q"] > 1:
            out.add(("blocks", "Q>1"))
            out.add(("blocks", "ragged") if p["ragged"] else ("blocks", "full_last"))
        if p["clause_binds"]: out.add(("blocks", "clause_binds"))
        out.add(("streams", "side_by_side") if p["side_by_side"] else ("streams", "shared"))
        if p["nw"] == 0: out.add(("wires", "nw0"))
        if p["nh"] == 0: out.add(("wires", "nh0"))
    if len({p["logM"] for p in plans if p["qcnt"]}) > 1: out.add(("blocks", "ranks_differ_logM"))
    if SPMV_LONG in case.get("row_lens", ()): out.add(("spmv", "rowwise", "at_limit"))
    if case.get("row_max", 0) > SPMV_LONG: out.add(("spmv", "rowwise", "long"))
    if case.get("col_max", 0) > SPMV_LONG: out.add(("spmv", "colwise", "long"))
    if case.get("unused_stmt"): out.add(("wires", "unused_stmt"))
    if case.get("unused_wit"): out.add(("wires", "unused_wit"))
    if l > 1: out.add(("wires", "l>1"))
    return out
