"""Python-integer restatement of the device R1CS -> QAP build (csrc/zkt_qap.hip), step for step:
     t(x)   = prod_{i=1..n} (x - i)
     q_j    = t / (x - j) by synthetic division (c = t[k] + c j, q_j[k-1] = c for k = n .. 1)            k_qap_basis
     w_j    = (-1)^(n-j) / ((j-1)! (n-j)!), the factorials from two prefix products and one inversion      k_qap_weights
     u_i    = sum over the stored entries (j, i, v) of column i of (v mod r) w_j q_j                       k_qap_scale, k_qap_columns
and the case list tests/test_gpu_qap_build.py runs.  tests/test_qap_build_model.py checks this file against tests/qap_util.py (the reference's own
interpolation) and the case list against the constants the source holds.  TEST INFRASTRUCTURE."""
import os, re
import numpy as np
from zkt_testlib import R, ROOT, ints_to_arr, SplitMix64

SRC = os.path.join(ROOT, "zk-toolkit_amd", "csrc", "zkt_qap.hip")
QAP_TPB = 256
QAP_MAX_N = 8192
QAP_MAX_CELLS = 1 << 26
BASIS_CHUNK = None          # k_qap_basis runs the whole division in one lane: no chunk length


def model_constants():
    return {"QAP_TPB": QAP_TPB, "QAP_MAX_N": QAP_MAX_N, "QAP_MAX_CELLS": QAP_MAX_CELLS, "BASIS_CHUNK": BASIS_CHUNK}


def library_constants():
    """the same constants as the library source and the header write them"""
    with open(SRC) as f:
        text = f.read()
    def one(pattern, where=text):
        m = re.findall(pattern, where, flags=re.M)
        assert len(m) == 1, (pattern, m)
        return m[0]
    tpb = int(one(r"^static constexpr int QAP_TPB = (\d+);"))
    one(r"const size_t j = \(size_t\)blockIdx\.x \* QAP_TPB \+ threadIdx\.x; if \(j >= n\) return;")               # the basis kernel: one lane per row
    one(r"const size_t cell = \(size_t\)blockIdx\.x \* QAP_TPB \+ threadIdx\.x; if \(cell >= cells\) return;")     # the accumulate kernel: one lane per cell
    chunk = re.findall(r"^static constexpr \w+ QAP_\w*CHUNK\w* = (\d+);", text, flags=re.M)                         # a chunked division would name its length so
    with open(os.path.join(ROOT, "include", "zkt.h")) as f:
        hdr = f.read()
    max_n = int(one(r"^#define ZKT_QAP_MAX_N +\(\(size_t\)(\d+)\)", hdr))
    max_cells = 1 << int(one(r"^#define ZKT_QAP_MAX_CELLS +\(\(size_t\)1 << (\d+)\)", hdr))
    return {"QAP_TPB": tpb, "QAP_MAX_N": max_n, "QAP_MAX_CELLS": max_cells, "BASIS_CHUNK": int(chunk[0]) if chunk else None}


# ---- the algorithm ------------------------------------------------------------------------------------------------
def t_poly(n):
    t = [1]
    for i in range(1, n + 1):
        nxt = [0] * (len(t) + 1)
        for k, c in enumerate(t):
            nxt[k] = (nxt[k] - c * i) % R; nxt[k + 1] = (nxt[k + 1] + c) % R
        t = nxt
    return t


def basis_row(t, n, j):
    q = [0] * n; c = 0
    for k in range(n, 0, -1):
        c = (t[k] + c * j) % R; q[k - 1] = c
    return q


def weights(n):
    f = [max(i, 1) for i in range(n)]; g = [max(n - 1 - i, 1) for i in range(n)]
    for i in range(1, n): f[i] = f[i - 1] * f[i] % R; g[i] = g[i - 1] * g[i] % R          # f[i] = i!, g[i] = (n-1)! / (n-2-i)!
    inv_top = pow(f[n - 1], -1, R)
    inv_fact = lambda k: inv_top if k == n - 1 else inv_top * g[n - 2 - k] % R
    w = []
    for i in range(n):
        c = inv_fact(i) * inv_fact(n - 1 - i) % R
        w.append((R - c) % R if (n - 1 - i) & 1 else c)
    return w


def qap_build(n, cols, mats):
    """mats: three lists of stored entries (row, col, value), value any integer below 2^256, duplicates allowed.  Returns three lists of `cols` lists of n
    coefficients, low degree first."""
    t = t_poly(n); w = weights(n)
    basis = {}
    out = []
    for entries in mats:
        P = [[0] * n for _ in range(cols)]
        for j, i, v in entries:
            c = (v % R) * w[j] % R
            if j not in basis: basis[j] = basis_row(t, n, j + 1)
            q = basis[j]; p = P[i]
            if c:
                for k in range(n): p[k] = (p[k] + c * q[k]) % R
        out.append(P)
    return out


def horner(p, x):
    acc = 0
    for c in reversed(p): acc = (acc * x + c) % R
    return acc


def dense_matrix(n, cols, entries):
    M = [[0] * cols for _ in range(n)]
    for j, i, v in entries: M[j][i] = (M[j][i] + v) % R
    return M


def entries_of(M):
    return [(j, i, v) for j, row in enumerate(M) for i, v in enumerate(row) if v % R]


def csr(n, entries):
    """stored entries in row-major order (as given within a row) -> (rowptr u64[n+1], col u32[nnz], val (nnz, 4) u64); the values keep their 256 bits"""
    rows = [[] for _ in range(n)]
    for j, i, v in entries: rows[j].append((i, v))
    rowptr, col, val = [0], [], []
    for r in rows:
        for i, v in r: col.append(i); val.append(v)
        rowptr.append(len(col))
    return np.array(rowptr, np.uint64), np.array(col if col else [0], np.uint32), ints_to_arr(val if val else [0], 4)


def qap_rs_circuit():
    """the 4-constraint circuit of the reference's test_r1cs_to_polynomial (qap.rs:229-317): x^3 + x + 5 = 35 with x = 3, wires [1, x, out, sym_1, y, sym_2]"""
    A = [[0, 1, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0], [0, 1, 0, 0, 1, 0], [5, 0, 0, 0, 0, 1]]
    B = [[0, 1, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0]]
    C = [[0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 1], [0, 0, 1, 0, 0, 0]]
    return A, B, C, [1, 3, 35, 9, 27, 30]


# ---- the GPU test's cases -------------------------------------------------------------------------------------------
# (n, cols): n = 1, 2, 3 and both sides of one and of two blocks of k_qap_basis; cols below, at and above a multiple of QAP_TPB; cells = cols * n at and off a
# multiple of QAP_TPB; polynomials shorter than a block that straddle block boundaries of k_qap_columns
CASES = [(1, 4), (2, 5), (3, 7), (20, 22), (255, 6), (256, 255), (257, 256), (513, 257)]
EDGE_VALUES = [R, R + 1, (1 << 256) - 1, R - 1]


ACTIVE_COLUMNS = 12


def case_matrices(n, cols, seed=11):
    """Three matrices for a case, as stored-entry lists: column 0 holds every row (the "one" wire), column cols // 2 and the last column are empty, one
    (row, col) entry is stored twice, and r, r + 1, 2^256 - 1 and r - 1 are among the values.  Besides column 0 at most ACTIVE_COLUMNS + 2 columns hold
    entries — spread from the first to the last free one, with the two neighbours of the empty middle column among them — so that the model's and the
    definition's cost stay with n, not with cols; every other column is a wire in no constraint."""
    assert cols >= 4
    rng = SplitMix64(seed * 1000003 + n * 131 + cols)
    empty = {cols // 2, cols - 1}
    free = [i for i in range(1, cols) if i not in empty]
    active = sorted({free[(len(free) - 1) * t // (ACTIVE_COLUMNS - 1)] for t in range(ACTIVE_COLUMNS)} | ({cols // 2 - 1, cols // 2 + 1} & set(free)))
    mats = []
    for m in range(3):
        ent = [(j, 0, rng.below(R)) for j in range(n)]
        for q in range(2 * min(n, len(active)) + 4):
            ent.append((rng.below(n), active[rng.below(len(active))], rng.below(R)))
        for q, v in enumerate(EDGE_VALUES):
            ent.append(((q + m) % n, active[(q * 7 + m) % len(active)], v))
        j, i, v = ent[n + 1]
        ent.append((j, i, rng.below(R)))                                  # the duplicated (row, col)
        ent.sort(key=lambda e: e[0])                                        # row-major, the order within a row as drawn
        mats.append(ent)
    return mats


CELLS = ["n=1", "n=2", "n=3", "n<tpb", "n=tpb-1", "n=tpb", "n=tpb+1", "n>2tpb", "cols<tpb", "cols=tpb", "cols>tpb", "cells%tpb=0", "cells%tpb!=0",
         "column_straddles_block", "block_holds_several_columns", "column_spans_blocks"]


def census(n, cols, tpb=QAP_TPB):
    c = set()
    if n in (1, 2, 3): c.add(f"n={n}")
    if n < tpb: c.add("n<tpb")
    if n == tpb - 1: c.add("n=tpb-1")
    if n == tpb: c.add("n=tpb")
    if n == tpb + 1: c.add("n=tpb+1")
    if n > 2 * tpb: c.add("n>2tpb")
    c.add("cols<tpb" if cols % tpb and cols < tpb else "cols=tpb" if cols % tpb == 0 else "cols>tpb")
    c.add("cells%tpb=0" if (cols * n) % tpb == 0 else "cells%tpb!=0")
    if n < tpb and tpb % n and cols * n > tpb: c.add("column_straddles_block")
    if 2 * n <= tpb: c.add("block_holds_several_columns")
    if n > tpb: c.add("column_spans_blocks")
    return c
