"""CPU checks of tests/qap_build_model.py: it equals the test-side restatement of the reference's interpolation (tests/qap_util.py) on the reference's own
circuits, its polynomials take the matrix entries as values on {1..n} for every case the GPU test runs, its constants are the ones csrc/zkt_qap.hip and
include/zkt.h hold, and the case list reaches every cell of the plan — checked before anything runs on a GPU."""
import numpy as np
import pytest
import qap_build_model as Q
from qap_util import qap_from_r1cs, example_cubic, chain_circuit, bits_circuit

R = Q.R


CIRCUITS = {"example_cubic": lambda: example_cubic()[:4], "chain20": lambda: chain_circuit(20)[:4], "bits33": lambda: bits_circuit(33)[:4], "qap_rs": Q.qap_rs_circuit}


@pytest.mark.parametrize("name", list(CIRCUITS))
def test_model_equals_the_reference_interpolation(name):
    A, B, C, wit = CIRCUITS[name]()
    n, cols = len(A), len(A[0])
    ui, vi, wi, _, t = qap_from_r1cs(A, B, C, wit)
    got = Q.qap_build(n, cols, [Q.entries_of(M) for M in (A, B, C)])
    pad = lambda P: [p + [0] * (n - len(p)) for p in P]
    assert got == [pad(ui), pad(vi), pad(wi)]
    assert Q.t_poly(n) == t


def test_the_qap_rs_witness_satisfies_its_circuit():
    A, B, C, w = Q.qap_rs_circuit()
    dot = lambda row: sum(a * b for a, b in zip(row, w)) % R
    assert all(dot(a) * dot(b) % R == dot(c) for a, b, c in zip(A, B, C))


@pytest.mark.parametrize("n,cols", Q.CASES)
def test_polynomials_take_the_matrix_entries_on_the_domain(n, cols):
    """u_i(j) = M[j][i] for every j in 1..n, on every column of every matrix"""
    mats = Q.case_matrices(n, cols)
    polys = Q.qap_build(n, cols, mats)
    for ent, P in zip(mats, polys):
        M = Q.dense_matrix(n, cols, ent)
        assert len(P) == cols and all(len(p) == n for p in P)
        live = [i for i in range(cols) if any(P[i]) or any(M[j][i] for j in range(n))]         # every other column: the zero polynomial through zeros
        acc = np.zeros((len(live), n), dtype=object); xs = np.array(range(1, n + 1), dtype=object)[None, :]
        for k in range(n - 1, -1, -1):                                                          # Horner, all live columns and all points at once
            acc = (acc * xs + np.array([P[i][k] for i in live], dtype=object)[:, None]) % R
        assert acc.tolist() == [[M[j][i] for j in range(n)] for i in live], (n, cols)
        assert 0 in live and len(live) >= min(3, cols - 2)


@pytest.mark.parametrize("n,cols", Q.CASES)
def test_case_matrices_hold_what_the_gpu_test_needs(n, cols):
    for ent in Q.case_matrices(n, cols):
        by_col = {}
        for j, i, v in ent: by_col.setdefault(i, []).append(j)
        assert sorted(by_col[0]) == list(range(n))                                     # the "one" wire: every row
        assert cols // 2 not in by_col and cols - 1 not in by_col                      # an empty column in the middle, an empty last column
        assert 0 < cols // 2 < cols - 1
        pairs = [(j, i) for j, i, _ in ent]
        assert len(pairs) - len(set(pairs)) >= 1                                       # a duplicated (row, col)
        assert set(Q.EDGE_VALUES) <= {v for _, _, v in ent}
        assert [e[0] for e in ent] == sorted(e[0] for e in ent)                        # row-major: a valid CSR order
    assert Q.EDGE_VALUES == [R, R + 1, (1 << 256) - 1, R - 1]


def test_n_equal_one_is_the_entry_itself():
    mats = Q.case_matrices(1, 4)
    for ent, P in zip(mats, Q.qap_build(1, 4, mats)):
        M = Q.dense_matrix(1, 4, ent)
        assert P == [[M[0][i]] for i in range(4)]


def test_weights_are_the_inverse_derivative_of_t():
    for n in (1, 2, 3, 8, 21):
        for j in range(1, n + 1):
            d = 1
            for i in range(1, n + 1):
                if i != j: d = d * (j - i) % R
            assert Q.weights(n)[j - 1] * d % R == 1, (n, j)


def test_model_constants_are_the_source_s():
    assert Q.library_constants() == Q.model_constants()


def test_gpu_cases_reach_every_cell():
    src = Q.library_constants()
    tpb = src["QAP_TPB"]
    ns = {n for n, _ in Q.CASES}
    assert {1, 2, 3, 255, 256, 257, 513} <= ns
    assert {tpb - 1, tpb, tpb + 1, 2 * tpb + 1} <= ns
    colset = {c for _, c in Q.CASES}
    assert any(c % tpb == tpb - 1 for c in colset) and any(c % tpb == 0 for c in colset) and any(c % tpb == 1 and c > tpb for c in colset)
    reached = set().union(*(Q.census(n, c, tpb) for n, c in Q.CASES))
    assert reached <= set(Q.CELLS), reached - set(Q.CELLS)
    assert not set(Q.CELLS) - reached, sorted(set(Q.CELLS) - reached)
    chunk = src["BASIS_CHUNK"]
    if chunk is not None:                                                                # a chunked division: both sides of its length are cases
        assert {chunk - 1, chunk, chunk + 1} <= ns
    assert all(n <= src["QAP_MAX_N"] and n * c <= src["QAP_MAX_CELLS"] and c >= 4 for n, c in Q.CASES)
