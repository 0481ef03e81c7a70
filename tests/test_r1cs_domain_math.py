"""The identity behind the scalable Groth16 path: on the reference's interpolation domain {1..n}
(qap.rs:33-97) the proof's Fr quantities a(x), b(x), h(x) t(x) can be computed from (A w, B w, C w) alone — no
coefficient-form polynomials.  Checked in python integers against the dense QAP of tests/qap_util.py."""
import pytest
from zkt_testlib import R, SplitMix64
import numpy as np
from zkt_testlib import ints_to_arr
from qap_util import example_cubic, chain_circuit, chain_circuit_sparse, qap_from_r1cs, domain_model, groth16_proof_scalars
from r1cs_plan_model import block_plan as _block_plan


def _eval(p, x):
    acc = 0
    for c in reversed(p): acc = (acc * x + c) % R
    return acc


@pytest.mark.parametrize("case", ["cubic", "chain1", "chain2", "chain7", "chain16"])
def test_domain_form_equals_dense_qap(case):
    A, B, C, w, l = example_cubic() if case == "cubic" else chain_circuit(int(case[5:]))
    ui, vi, wi, h, t = qap_from_r1cs(A, B, C, w)
    x = SplitMix64(99).below(R - 100) + 50
    comb = lambda P: sum(w[i] * _eval(P[i], x) for i in range(len(w))) % R
    ax, bx, htx = domain_model(A, B, C, w, x)
    assert ax == comb(ui) and bx == comb(vi)
    assert htx == _eval(h, x) * _eval(t, x) % R


@pytest.mark.parametrize("n", [1, 2, 12, 40])
def test_proof_scalars_in_linear_time_equal_the_coefficient_form(n):
    """groth16_proof_scalars (the O(n) python-integer checker of the full-size GPU tests: discrete logarithms of A, B, C from the trapdoor) against the
    reference's own coefficient-form prover (prover.rs:96-147 over the dense QAP of qap_from_r1cs; crs.rs:65-121 for uvw_wit and xt_by_delta)."""
    mats, wires, l, m = chain_circuit_sparse(n, seed=11)
    A, B, C, wit, l2 = chain_circuit(n, seed=11)
    toi = lambda a: [int.from_bytes(np.ascontiguousarray(v).tobytes(), "little") for v in np.asarray(a).reshape(-1, 4)]
    assert toi(wires) == [v % R for v in wit] and l == l2
    rng = SplitMix64(5 + n); fr = lambda v: ints_to_arr([v], 4)
    trap = [fr(rng.below(R - 1) + 1) for _ in range(5)]; r = fr(rng.below(R - 1) + 1); s = fr(rng.below(R - 1) + 1)
    got = groth16_proof_scalars(mats, wires, l, trap, r, s)
    alpha, beta, gamma, delta, x = [toi(t)[0] for t in trap]
    rr, ss = toi(r)[0], toi(s)[0]
    ui, vi, wi, h, t = qap_from_r1cs(A, B, C, wit)
    As = (alpha + sum(wit[i] * _eval(ui[i], x) for i in range(m + 1)) + rr * delta) % R
    Bs = (beta + sum(wit[i] * _eval(vi[i], x) for i in range(m + 1)) + ss * delta) % R
    di = pow(delta, -1, R)
    Cs = (sum(wit[i] * (beta * _eval(ui[i], x) + alpha * _eval(vi[i], x) + _eval(wi[i], x)) for i in range(l + 1, m + 1)) * di
          + _eval(h, x) * _eval(t, x) * di + ss * As + rr * Bs - rr * ss * delta) % R
    assert got == (As, Bs, Cs)


@pytest.mark.parametrize("n,nshards", [(2, 1), (5, 1), (37, 1), (1025, 1), (1500, 1), (1500, 3), (2600, 5), (2600, 8), (40, 39)])
def test_blocked_convolution_gives_every_rank_its_quotient_values(n, nshards):
    """k_recip_blocks / k_prep_blocks / k_sum_blocks in python integers: S(s) = sum_{j=1..n} f_j / (n + s - j) for the rank's s = s0 .. s0 + cnt - 1 equals entry s - s0 of
    sum_q (block q of f, zero-padded to M) (*) (kernel slice q) as CYCLIC convolutions of size M = 2 Bi — the overlap-save identity the sharded quotient stage rests on
    (prover.rs:64-71 divides in coefficient form; qap.rs:33-97 fixes the domain {1..n}).  The cyclic convolutions are evaluated directly (no transform), sampled outputs."""
    rng = SplitMix64(1000 * n + nshards)
    f = [0] + [rng.below(R) for _ in range(n)]                        # f[j], j = 1..n
    inv = lambda d: pow(d, -1, R)
    g = lambda d: inv(d) if 1 <= d <= 2 * n - 1 else 0
    seen = 0
    for shard in range(nshards):
        cnt, s0, Bi, M, Q = _block_plan(n, nshards, shard)
        assert cnt <= Bi and Q * Bi >= n
        if cnt == 0: continue
        # kernel slices exactly as k_recip_blocks lays them out
        K = []
        for q in range(Q):
            base = n + s0 - 1 - q * Bi
            K.append({e: g(base + e) for e in range(cnt)} | {e: g(base - (M - e)) for e in range(M - Bi + 1, M)})
        X = [[f[q * Bi + 1 + e] if e < Bi and q * Bi + e < n else 0 for e in range(M)] for q in range(Q)]
        for u in sorted({0, cnt - 1, cnt // 2, rng.below(cnt)}):     # sampled outputs: a cyclic convolution entry costs M products per block
            got = 0
            for q in range(Q):
                for v in range(Bi):                                   # the upper half of a block is zero padding
                    if X[q][v]: got += X[q][v] * K[q].get((u - v) % M, 0)
            s = s0 + u
            want = sum(f[j] * inv(n + s - j) for j in range(1, n + 1)) % R
            assert got % R == want, (shard, u)
        seen += cnt
    assert seen == max(n - 1, 0)                                      # the ranks' ranges tile s = 1 .. n-1


def _dense(M, n, cols):
    rowptr, col, val = M
    vals = [int.from_bytes(np.ascontiguousarray(v).tobytes(), "little") for v in val]
    D = [[0] * cols for _ in range(n)]
    for j in range(n):
        for k in range(int(rowptr[j]), int(rowptr[j + 1])): D[j][int(col[k])] = (D[j][int(col[k])] + vals[k]) % R
    return D


@pytest.mark.parametrize("n,opts", [(1, {}), (2, {"l": 1}), (7, {"unused_stmt": True, "unused_wit": True}), (12, {"l": 4}), (9, {"all_public": True}),
                                    ("40:13", {"unused_wit": True})])
def test_asymmetric_circuit_and_its_models_equal_the_coefficient_form(n, opts):
    """qap_util.asym_circuit_sparse is satisfied by its witness, its A and B differ, and the python-integer models the GPU plan tests check against —
    groth16_proof_scalars over row_dots and uvw_stmt_scalars (vk.g1_uvw_stmt) — equal the reference's coefficient-form prover and CRS (prover.rs:96-147,
    crs.rs:65-121) over the dense QAP.  "40:13": the first 13 constraints of a 40-constraint circuit (qap_util.prefix)."""
    from qap_util import asym_circuit_sparse, prefix, row_dots, uvw_stmt_scalars, lagrange_at
    if isinstance(n, str):
        big, n = (int(v) for v in n.split(":"))
        mats, wires, l, m = prefix(asym_circuit_sparse(big, seed=big, **opts), n)
    else:
        mats, wires, l, m = asym_circuit_sparse(n, seed=n, **opts)
    toi = lambda a: [int.from_bytes(np.ascontiguousarray(v).tobytes(), "little") for v in np.asarray(a).reshape(-1, 4)]
    wit = toi(wires)
    assert len(wit) == m + 1 and l == (m if opts.get("all_public") else opts.get("l", 3))
    A, B, C = (_dense(M, n, m + 1) for M in mats)
    dot = lambda D: [sum(c * w for c, w in zip(row, wit)) % R for row in D]
    assert [a * b % R for a, b in zip(dot(A), dot(B))] == dot(C), "witness does not satisfy the circuit"
    if n > 1: assert A != B
    for k, flag in ((l, "unused_stmt"), (l + 3, "unused_wit")):
        if opts.get(flag): assert all(row[k] == 0 for D in (A, B, C) for row in D)
    rows = row_dots(mats, wires, l)
    assert [list(v) for v in rows[0]] == [dot(A), [sum(c * w for c, w in list(zip(row, wit))[l + 1:]) % R for row in A]]
    rng = SplitMix64(77 + n); fr = lambda v: ints_to_arr([v], 4)
    trap = [fr(rng.below(R - 1) + 1) for _ in range(5)]; r = fr(rng.below(R - 1) + 1); s = fr(rng.below(R - 1) + 1)
    alpha, beta, gamma, delta, x = [toi(t)[0] for t in trap]
    rr, ss = toi(r)[0], toi(s)[0]
    ui, vi, wi, h, t = qap_from_r1cs(A, B, C, wit)
    As = (alpha + sum(wit[i] * _eval(ui[i], x) for i in range(m + 1)) + rr * delta) % R
    Bs = (beta + sum(wit[i] * _eval(vi[i], x) for i in range(m + 1)) + ss * delta) % R
    di = pow(delta, -1, R)
    Cs = (sum(wit[i] * (beta * _eval(ui[i], x) + alpha * _eval(vi[i], x) + _eval(wi[i], x)) for i in range(l + 1, m + 1)) * di
          + _eval(h, x) * _eval(t, x) * di + ss * As + rr * Bs - rr * ss * delta) % R
    Lx = lagrange_at(n, x)
    assert groth16_proof_scalars(mats, wires, l, trap, r, s) == (As, Bs, Cs)
    assert groth16_proof_scalars(mats, wires, l, trap, r, s, Lx=Lx, rows=rows) == (As, Bs, Cs)
    gi = pow(gamma, -1, R)
    want = [(beta * _eval(ui[i], x) + alpha * _eval(vi[i], x) + _eval(wi[i], x)) * gi % R for i in range(l + 1)]
    assert uvw_stmt_scalars(mats, l, trap) == want == uvw_stmt_scalars(mats, l, trap, Lx=Lx)
    if opts.get("unused_stmt"): assert want[l] == 0


def test_asymmetric_circuit_long_rows():
    """long_rows: rows 4098 and 4099 of A hold 4096 and 4097 terms, of B 4097 and 4096, every wire once, and the witness still satisfies every row"""
    from qap_util import asym_circuit_sparse, row_dots, LONG_ROWS_AT
    n = LONG_ROWS_AT + 9
    mats, wires, l, m = asym_circuit_sparse(n, seed=5, long_rows=True)
    for (rowptr, col, _), want in zip(mats[:2], ((4096, 4097), (4097, 4096))):
        lens = np.diff(rowptr.astype(np.int64))
        assert tuple(lens[LONG_ROWS_AT:LONG_ROWS_AT + 2]) == want and lens.max() == 4097 and (lens[:LONG_ROWS_AT] <= 4).all()
        for j in (LONG_ROWS_AT, LONG_ROWS_AT + 1):
            c = col[int(rowptr[j]):int(rowptr[j + 1])]
            assert len(set(c.tolist())) == len(c) and c.max() < l + 3 + j
    (az, _), (bz, _), (cz, _) = row_dots(mats, wires, l)
    assert list(az * bz % R) == list(cz)
