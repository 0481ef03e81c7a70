"""The discrete-log model of Bulletproofs (tests/bp_model.py) pinned to the oracle, bit for bit, at small n: verdict, out_pts
(A, S, T1, T2, P, written before the decision, so compared on rejection too) and the inner-product trace (L, R, P' per level),
for every instance kind the GPU tests use.  CPU only: the generators come from the oracle's scalar multiplication."""
import numpy as np
import pytest
from zkt_testlib import oracle, ptr, ints_to_arr, SplitMix64, SECP_N, SECP_GEN, py_secp_mul, secp_arr
import bp_model as M

O = oracle()
SIZES = (1, 2, 4, 8, 16)


def gens(n, seed):
    """2n + 3 generators from known dlogs through the oracle (as test_oracle_protocols.ipa_instance): (Gens, gg, hh, g, h, u)"""
    rng = SplitMix64(seed)
    ks = [rng.below(SECP_N - 1) + 1 for _ in range(2 * n + 3)]
    g0 = np.zeros((1, 9), np.uint64); O.zkto_secp_generator(ptr(g0))
    pts = np.zeros((2 * n + 3, 9), np.uint64)
    assert O.zkto_secp_mul_batch(ptr(np.repeat(g0, 2 * n + 3, axis=0)), ptr(ints_to_arr(ks, 4)), 4, ptr(pts), 2 * n + 3, 8) == 0
    G = M.Gens(ks[2 * n], ks[2 * n + 1], ks[2 * n + 2], ks[:n], ks[n:2 * n])
    return G, pts[:n].copy(), pts[n:2 * n].copy(), pts[2 * n:2 * n + 1].copy(), pts[2 * n + 1:2 * n + 2].copy(), pts[2 * n + 2:].copy()


def test_points_helper_matches_oracle():
    ks = [0, 1, 2, SECP_N - 1, 0xDEADBEEF]
    got = np.zeros((len(ks), 9), np.uint64)
    g0 = np.zeros((1, 9), np.uint64); O.zkto_secp_generator(ptr(g0))
    assert (g0 == secp_arr([SECP_GEN])).all()
    assert O.zkto_secp_mul_batch(ptr(np.repeat(g0, len(ks), axis=0)), ptr(ints_to_arr(ks, 4)), 4, ptr(got), len(ks), 1) == 0
    assert (M.points(ks) == got).all()
    assert M.points([0])[0, 8] == 1


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", M.KINDS)
def test_range_proof_model_vs_oracle(n, kind):
    G, gg, hh, g, h, u = gens(n, 300 + n)
    I = M.rp_instance(kind, n, 1000 * n + M.KINDS.index(kind))
    V = M.points([I.V(G)])
    if kind == "v_inf": assert V[0, 8] == 1
    if kind == "y_one": assert I.rndi[2] == 1
    for use_ipa in (0, 1):
        ok, pts = M.range_proof(n, I.V(G), I.aLi, I.gammai, G, I.rndi, use_ipa, I.xsi)
        op = np.zeros((5, 9), np.uint64)
        want = O.zkto_bp_range_proof(n, ptr(V), ptr(I.aL), ptr(I.gamma), ptr(g), ptr(h), ptr(gg), ptr(hh), use_ipa, ptr(I.rnd), ptr(u), ptr(I.xs), ptr(op))
        assert want == int(ok), f"{kind} use_ipa={use_ipa}: model verdict {ok}, oracle {want}"
        assert ok == M.EXPECT[kind], f"{kind} does not give the verdict it is built for"
        assert (M.points(pts) == op).all(), f"{kind} use_ipa={use_ipa}: A, S, T1, T2, P"


@pytest.mark.parametrize("n", SIZES)
def test_ipa_model_vs_oracle(n):
    G, gg, hh, g, h, u = gens(n, 700 + n)
    I = M.ipa_instance(n, 70 + n, G)
    lv = M.levels_of(n) if n > 1 else 0
    cases = [("honest", I.ai, I.P, True)]
    for j in sorted({0, n // 2 - 1, n // 2, n - 1} - {-1}):
        a2 = list(I.ai); a2[j] = (a2[j] + 1) % SECP_N
        cases.append((f"a[{j}] + 1", a2, I.P, False))
    cases.append(("P + u", I.ai, (I.P + G.u) % SECP_N, False))
    for name, ai, P, expect in cases:
        ok, trace = M.ipa(n, G.gg, G.hh, G.u, P, ai, I.bi, I.xsi)
        assert ok == expect, name
        assert len(trace) == 3 * lv
        ot = np.zeros((max(3 * lv, 1), 9), np.uint64)
        want = O.zkto_bp_ipa(n, ptr(gg), ptr(hh), ptr(u), ptr(M.points([P])), ptr(ints_to_arr(ai, 4)), ptr(I.b), ptr(I.xs), ptr(ot))
        assert want == int(ok), name
        if lv: assert (M.points(trace) == ot).all(), f"{name}: trace"
