"""The host plan of the Groth16 R1CS prover (tests/r1cs_plan_model.py) checked without a GPU: its constants are the library's, every transform size's
stage groups move data exactly as the textbook radix-2 transforms do, and the GPU cases of tests/test_gpu_r1cs_plans.py reach every cell of the plan."""
import numpy as np
import pytest
from zkt_testlib import R, SplitMix64
import r1cs_plan_model as pm


def test_constants_are_the_librarys():
    assert pm.library_constants() == pm.model_constants()
    assert 2 * pm.MAX_N + 1 <= pm.SC_TILE ** 2 < 2 * (pm.MAX_N + 1) + 1          # the largest n whose 2n + 1 factorials fit two levels of scan tiles
    assert pm.scan_kind(2 * pm.MAX_N + 1) != "limit" and pm.scan_kind(2 * (pm.MAX_N + 1) + 1) == "limit"
    assert pm.plan(pm.MAX_N, 1, pm.MAX_N)["logM"] == pm.MAX_LOGM


@pytest.mark.parametrize("logN", range(1, pm.MAX_LOGM + 1))
def test_stage_groups_are_the_textbook_transform(logN):
    """the groups partition the stages, each tile fits the 1024-element LDS and the launches' tiles partition the array, and k_ntt_group's addressing
    (restated over every block with numpy) gives each stage exactly the textbook butterflies and twiddle exponents, in the order DIF / DIT run them"""
    g = pm.ntt_groups(logN)
    assert [lo for lo, _, _ in g] == list(np.cumsum([0] + [c for _, c, _ in g])[:-1]) and sum(c for _, c, _ in g) == logN
    N = 1 << logN
    for lo, cnt, cbits in g:
        assert 1 <= cnt <= (pm.NTT_TILE_LOG if lo == 0 else pm.NTT_MAX_STAGES) and cnt + cbits <= pm.NTT_TILE_LOG and cbits <= lo
        assert lo == 0 or cbits >= min(2, lo)                                      # >= 4 adjacent columns once there are that many
        for batch in ((1, 3) if logN <= 12 else (1,)):
            tiles = pm.group_tiles(logN, lo, cnt, cbits, batch)
            assert (np.sort(tiles.ravel()) == np.arange(batch * N)).all()         # every element in exactly one tile of the launch
        for t in range(cnt):
            u, v, e = (x.ravel() for x in pm.group_butterflies(logN, lo, cnt, cbits, t))
            tu, tv, te = pm.textbook_stage(logN, lo + t)
            order = np.argsort(u)
            assert (u[order] == tu).all() and (v[order] == tv).all() and (e[order] == te).all(), (lo, cnt, cbits, t)
            assert e.max(initial=0) < max(N // 2, 1)                              # inside the table of M/2 twiddles
    for dif in (True, False):
        s = [s for _, _, s in pm.stage_order(logN, dif)]
        assert s == (list(range(logN - 1, -1, -1)) if dif else list(range(logN)))


@pytest.mark.parametrize("logN", [1, 2, 3, 5, 8, 10, 11, 12])
def test_transform_through_the_groups_is_the_dft(logN):
    """python-int DIF through the groups' addressing = the DFT in bit-reversed order (sampled outputs); DIT with w^-1 through them brings it back times N"""
    N = 1 << logN
    w = pow(7, (R - 1) >> logN, R)
    assert pow(w, N, R) == 1 and (N == 1 or pow(w, N // 2, R) != 1)
    rng = SplitMix64(logN)
    a = [rng.below(R) for _ in range(N)]
    A = pm.ntt_through_groups(a, logN, w, R, dif=True)
    for k in sorted({0, 1, N - 1, N // 2, rng.below(N), rng.below(N)}):
        assert A[pm.bitrev(k, logN)] == sum(x * pow(w, i * k, R) for i, x in enumerate(a)) % R, k
    back = pm.ntt_through_groups(A, logN, pow(w, -1, R), R, dif=False)
    assert back == [x * N % R for x in a]


def test_launches_of_one_proof():
    """grid, ny and mulvec of every launch: setup transforms Q slices of one array, a proof Q blocks of three arrays forward (the last launch multiplies by
    the kernel spectrum) and one block of three arrays back"""
    for n, W in [(1, 1), (5, 1), (4097, 1), (9000, 16), (5, 5), (2 ** 20 + 2, 8)]:
        for k in range(W):
            p = pm.plan(n, 1, n + 1, k, W)
            L = pm.ntt_launches(p)
            g = pm.ntt_groups(p["logM"])
            setup = [x for x in L if x[0] == "setup_fwd"]; fwd = [x for x in L if x[0] == "prove_fwd"]; inv = [x for x in L if x[0] == "prove_inv"]
            assert [x[1:4] for x in setup] == list(reversed(g))
            for d, lo, cnt, cbits, grid, ny, mulvec in L:
                batch = 1 if d == "prove_inv" else p["Q"]
                assert grid << (cnt + cbits) == batch * p["M"] and ny == (1 if d == "setup_fwd" else 3)
                assert mulvec == (d == "prove_fwd" and lo == 0)
            if p["qcnt"]:
                assert [x[1:4] for x in fwd] == list(reversed(g)) and [x[1:4] for x in inv] == g and fwd[-1][-1]
            else:
                assert not fwd and not inv


def test_block_plans():
    """Bi >= cnt, the Q blocks cover the n inputs, the ranks' ranges tile the three sets, the clause, the stream layout"""
    for n in list(range(1, 70)) + [1023, 1024, 1025, 4096, 4097, 9000, 2 ** 20 + 2]:
        for W in sorted({1, 2, 3, 7, 16, n if n < 5000 else 8}):
            if W > n: continue
            ps = [pm.plan(n, 2, n + 5, k, W) for k in range(W)]
            for key in ("A", "C1", "C2"):
                assert [p[key][0] for p in ps[1:]] == [p[key][1] for p in ps[:-1]] and ps[0][key][0] == 0 and ps[-1][key][1] == ps[0]["n" + key]
            assert sum(p["qcnt"] for p in ps) == max(n - 1, 0)
            for p in ps:
                assert p["qcnt"] <= p["Bi"] and p["Q"] * p["Bi"] >= n and (p["Q"] - 1) * p["Bi"] < n or not p["qcnt"]
                assert p["Bi"] >= min(n, 1 << (pm.SMALL_LOGM - 1))
                assert p["clause_binds"] == (p["logM"] > 1 and (1 << (p["logM"] - 2)) >= p["qcnt"])


def test_scan_tiles():
    assert [pm.scan_kind(k) for k in (1, 2048, 2049, 4096, 4097, 4098, 2048 * 2048, 2048 * 2048 + 1)] == \
        ["one_tile", "one_tile", "tail1", "exact", "tail1", "ragged", "exact", "limit"]
    p = pm.plan(1024, 1, 1025)
    assert pm.scan_calls(p) == {"fact": 2049, "pre": 2047, "tw": 1024, "twinv": 1024}


def test_case_facts_match_the_circuit():
    """the facts test_gpu_r1cs_plans.case() states about a prefix of its circuit (layout, row lengths, the long "one" column) hold for a circuit built
    with the same options"""
    import test_gpu_r1cs_plans as G
    from qap_util import asym_circuit_sparse, prefix
    c = asym_circuit_sparse(G.LONG_ROWS_AT + 40, seed=3, l=G.L_STMT, long_rows=True, unused_stmt=True, unused_wit=True)
    for n in (1, 5, G.LONG_ROWS_AT + 2, G.LONG_ROWS_AT + 40):
        mats, wires, l, m = prefix(c, n)
        f = G.case(n)
        assert (l, m) == (f["l"], f["m"])
        lens = np.concatenate([np.diff(M[0].astype(np.int64)) for M in mats])
        assert lens.max() <= f["row_max"] and (lens.max() > pm.SPMV_LONG) == (f["row_max"] > pm.SPMV_LONG) and set(f["row_lens"]) <= set(lens.tolist())
        assert max(np.bincount(mats[1][1][:int(mats[1][0][n])], minlength=m + 1)) >= f["col_max"]
        used = set(np.concatenate([M[1][:int(M[0][n])] for M in mats]).tolist())
        assert (l not in used) and (l + 3 not in used) and f["unused_stmt"] and f["unused_wit"]


def test_census_reaches_every_cell():
    """every cell of the plan (every launch shape of logM 1 .. 22, the block, scan, mat-vec, stream and wire cases, the refusals) is run by a GPU case"""
    import test_gpu_r1cs_plans as G
    reached = set()
    for c in G.CASES:
        got = pm.census(c)
        assert got <= pm.CELLS, got - pm.CELLS
        reached |= got
    assert not pm.CELLS - reached, sorted(pm.CELLS - reached)
    # the transform shapes that no test ran before these
    for lo, cnt, cbits in [(10, 2, 8), (10, 5, 5), (10, 6, 4), (18, 1, 9), (18, 2, 8), (18, 4, 6)]:
        assert ("ntt", "prove_fwd", lo, cnt, cbits) in reached
