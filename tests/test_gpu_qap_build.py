"""The R1CS -> QAP build on the GPU (zkt_qap_build / zkt_qap_create) against the python-integer model of tests/qap_build_model.py, every coefficient of every
column of every case, and the dense Groth16 path from a resident QAP (zkt_qap_quotient_resident, zkt_groth16_setup_resident, zkt_groth16_prove_resident)
against the host-array entry points and the sparse-R1CS prover: all comparisons are byte equality.  tests/test_qap_build_model.py proves on the CPU that the
model is the reference's interpolation and that the cases reach every cell of the plan."""
import ctypes, importlib
import numpy as np
import pytest
import qap_build_model as Q
from zkt_testlib import ptr, ints_to_arr, SplitMix64, R, G1W, G2W, ZKT_ERR_SHAPE
from qap_util import sparse_rows, sparse_struct, alloc_crs, example_cubic, chain_circuit, bits_circuit

pytestmark = pytest.mark.gpu
zk = importlib.import_module("zk-toolkit_amd")
ZKT_ERR_REMAINDER = zk.ZKT_ERR_REMAINDER
PAT = 0xABABABABABABABAB
fr = lambda v: ints_to_arr([v], 4)


@pytest.fixture(scope="module")
def L():
    zk.init()
    return zk.lib()


def refs(structs): return [ctypes.byref(s) for s in structs]


def build(L, n, cols, structs):
    out = [np.full((cols * n, 4), PAT, np.uint64) for _ in range(3)]
    zk.check(L.zkt_qap_build(n, cols, *refs(structs), *(ptr(o) for o in out)))
    return out


def create(L, n, cols, structs):
    h = ctypes.c_void_p()
    zk.check(L.zkt_qap_create(n, cols, *refs(structs), ctypes.byref(h)))
    assert h.value
    return h


def download(L, h, n, cols):
    out = [np.full((cols * n, 4), PAT, np.uint64) for _ in range(3)]
    zk.check(L.zkt_qap_download(h, *(ptr(o) for o in out)))
    return out


_model = {}


def model_case(n, cols):
    """the case's matrices and the model's answer, computed once"""
    if (n, cols) not in _model:
        mats = Q.case_matrices(n, cols)
        want = [ints_to_arr([c for p in P for c in p], 4) for P in Q.qap_build(n, cols, mats)]
        _model[(n, cols)] = (mats, want)
    return _model[(n, cols)]


@pytest.mark.parametrize("n,cols", Q.CASES)
def test_build_equals_the_model_in_full(L, n, cols):
    mats, want = model_case(n, cols)
    structs = [sparse_struct(*Q.csr(n, ent)) for ent in mats]
    got = build(L, n, cols, structs)
    for name, g, w in zip("uvw", got, want):
        if g.tobytes() != w.tobytes():
            bad = np.nonzero((g != w).any(axis=1))[0]
            raise AssertionError(f"{name}i, n = {n}, cols = {cols}: {len(bad)} of {cols * n} coefficients differ, first at column {bad[0] // n}, degree {bad[0] % n}")
    if n == 1:                                                            # u_i = [M[0][i]]
        for ent, g in zip(mats, got):
            assert g.tobytes() == ints_to_arr(Q.dense_matrix(1, cols, ent)[0], 4).tobytes()
    # the handle holds the same bytes; a download with one pointer NULL leaves the other two right
    h = create(L, n, cols, structs)
    try:
        for g, d in zip(got, download(L, h, n, cols)): assert g.tobytes() == d.tobytes()
        for k in range(3):
            out = [np.full((cols * n, 4), PAT, np.uint64) for _ in range(3)]
            ps = [ptr(o) for o in out]; ps[k] = None
            zk.check(L.zkt_qap_download(h, *ps))
            for j in range(3):
                assert (out[j] == np.uint64(PAT)).all() if j == k else out[j].tobytes() == got[j].tobytes()
    finally:
        L.zkt_qap_free(h)


def circuit_structs(A, B, C):
    return [sparse_struct(*sparse_rows(M)) for M in (A, B, C)]


@pytest.mark.parametrize("name,make", [("example_cubic", lambda: example_cubic()[:4]), ("qap_rs", Q.qap_rs_circuit)])
def test_reference_circuits_build_to_a_valid_qap(L, name, make):
    """QAP::build then QAP::is_valid (qap.rs:137-213): the quotient leaves no remainder"""
    A, B, C, wit = make()
    n, cols = len(A), len(A[0])
    h = create(L, n, cols, circuit_structs(A, B, C))
    try:
        hq = np.zeros((max(n - 1, 1), 4), np.uint64)
        zk.check(L.zkt_qap_quotient_resident(h, ptr(ints_to_arr(wit, 4)), ptr(hq)))
        bad = list(wit); bad[1] += 1
        assert L.zkt_qap_quotient_resident(h, ptr(ints_to_arr(bad, 4)), ptr(hq)) == ZKT_ERR_REMAINDER
    finally:
        L.zkt_qap_free(h)


@pytest.mark.parametrize("n", [20, 257])
def test_resident_quotient_equals_the_host_array_quotient(L, n):
    A, B, C, wit, l = chain_circuit(n)
    cols = n + 2
    h = create(L, n, cols, circuit_structs(A, B, C))
    try:
        u, v, w = download(L, h, n, cols)
        wires = ints_to_arr(wit, 4)
        want = np.full((n - 1, 4), PAT, np.uint64); got = np.full((n - 1, 4), PAT, np.uint64)
        zk.check(L.zkt_qap_quotient(ptr(u), ptr(v), ptr(w), cols, n, ptr(wires), ptr(want)))
        zk.check(L.zkt_qap_quotient_resident(h, ptr(wires), ptr(got)))
        assert got.tobytes() == want.tobytes() and not (got == np.uint64(PAT)).all()
        bad = list(wit); bad[3] = (bad[3] + 1) % R                       # one wire changed: the same remainder, reported the same way
        wires = ints_to_arr(bad, 4)
        want[:] = np.uint64(PAT); got[:] = np.uint64(PAT)
        assert L.zkt_qap_quotient(ptr(u), ptr(v), ptr(w), cols, n, ptr(wires), ptr(want)) == ZKT_ERR_REMAINDER
        idx = L.zkt_last_error_index()
        assert L.zkt_qap_quotient_resident(h, ptr(wires), ptr(got)) == ZKT_ERR_REMAINDER
        assert L.zkt_last_error_index() == idx
        assert got.tobytes() == want.tobytes()
    finally:
        L.zkt_qap_free(h)


def abc():
    return [np.full((1, G1W), PAT, np.uint64), np.full((1, G2W), PAT, np.uint64), np.full((1, G1W), PAT, np.uint64)]


@pytest.mark.parametrize("name,make", [("chain20", lambda: chain_circuit(20)), ("chain257", lambda: chain_circuit(257)), ("bits33", lambda: bits_circuit(33))])
def test_setup_and_prove_from_the_handle_end_to_end(L, name, make):
    A, B, C, wit, l = make()
    n, cols = len(A), len(A[0]); m = cols - 1
    structs = circuit_structs(A, B, C)
    rng = SplitMix64(len(name) * 977 + n)
    trap = [fr(rng.below(R - 1) + 1) for _ in range(4)] + [fr(rng.below(R - 3 * n) + 2 * n)]       # x outside {1 .. 2n-1}
    r, s = fr(rng.below(R - 1) + 1), fr(rng.below(R - 1) + 1)
    wires = ints_to_arr(wit, 4)
    h = create(L, n, cols, structs)
    try:
        u, v, w = download(L, h, n, cols)
        crs_h, buf_h = alloc_crs(n, l, m); crs_r, buf_r = alloc_crs(n, l, m)
        for b in list(buf_h.values()) + list(buf_r.values()): b[:] = np.uint64(PAT)
        zk.check(L.zkt_groth16_setup(ctypes.byref(crs_h), ptr(u), ptr(v), ptr(w), *[ptr(t) for t in trap]))
        zk.check(L.zkt_groth16_setup_resident(ctypes.byref(crs_r), h, *[ptr(t) for t in trap]))
        for k in buf_h: assert buf_r[k].tobytes() == buf_h[k].tobytes(), f"CRS field {k}"
        assert not (buf_r["g1_xi"] == np.uint64(PAT)).all()
        want, got = abc(), abc()
        zk.check(L.zkt_groth16_prove_qap(ctypes.byref(crs_h), ptr(u), ptr(v), ptr(w), ptr(wires), ptr(r), ptr(s), *[ptr(x) for x in want]))
        zk.check(L.zkt_groth16_prove_resident(ctypes.byref(crs_r), h, ptr(wires), ptr(r), ptr(s), *[ptr(x) for x in got]))
        for a, b, e in zip(got, want, "ABC"): assert a.tobytes() == b.tobytes(), f"proof element {e}"
        # the sparse-R1CS prover, from the same CSR, trapdoor, r and s
        vk, vbuf = alloc_crs(1, l, m); pk = ctypes.c_void_p()
        zk.check(L.zkt_groth16_setup_r1cs(n, l, m, *[ctypes.addressof(x) for x in structs], *[t.ctypes.data for t in trap], ctypes.addressof(vk), ctypes.addressof(pk)))
        try:
            sp = abc()
            zk.check(L.zkt_groth16_prove_r1cs(pk, wires.ctypes.data, r.ctypes.data, s.ctypes.data, *[x.ctypes.data for x in sp]))
        finally:
            L.zkt_groth16_pk_free(pk)
        for a, b, e in zip(got, sp, "ABC"): assert a.tobytes() == b.tobytes(), f"proof element {e} against the sparse-R1CS prover"
        stmt = ints_to_arr(wit[:l + 1], 4)
        assert L.zkt_groth16_verify(ctypes.byref(crs_r), *[ptr(x) for x in got], ptr(stmt), l + 1) == 1
        bad = stmt.copy(); bad[1, 0] ^= np.uint64(1)
        assert L.zkt_groth16_verify(ctypes.byref(crs_r), *[ptr(x) for x in got], ptr(bad), l + 1) == 0
        # a witness with one wire changed: the same ZKT_ERR_REMAINDER and index from both provers, outputs untouched
        w2 = list(wit); w2[3] = (w2[3] + 1) % R; wires2 = ints_to_arr(w2, 4)
        o1, o2 = abc(), abc()
        assert L.zkt_groth16_prove_qap(ctypes.byref(crs_h), ptr(u), ptr(v), ptr(w), ptr(wires2), ptr(r), ptr(s), *[ptr(x) for x in o1]) == ZKT_ERR_REMAINDER
        idx = L.zkt_last_error_index()
        assert L.zkt_groth16_prove_resident(ctypes.byref(crs_r), h, ptr(wires2), ptr(r), ptr(s), *[ptr(x) for x in o2]) == ZKT_ERR_REMAINDER
        assert L.zkt_last_error_index() == idx
        assert all((x == np.uint64(PAT)).all() for x in o1 + o2)
    finally:
        L.zkt_qap_free(h)


def test_a_handle_of_another_shape_is_a_shape_error(L):
    A, B, C, wit, l = chain_circuit(20)
    n, cols = 20, 22
    h = create(L, n, cols, circuit_structs(A, B, C))
    try:
        k = fr(5); wires = ints_to_arr(wit, 4)
        for cn, cm in ((n + 1, cols - 1), (n - 1, cols - 1), (n, cols), (n, cols - 2)):          # a wrong n; a wrong cols
            crs, buf = alloc_crs(cn, l, cm)
            for b in buf.values(): b[:] = np.uint64(PAT)
            assert L.zkt_groth16_setup_resident(ctypes.byref(crs), h, ptr(k), ptr(k), ptr(k), ptr(k), ptr(k)) == ZKT_ERR_SHAPE, (cn, cm)
            assert all((b == np.uint64(PAT)).all() for b in buf.values())
            out = abc()
            assert L.zkt_groth16_prove_resident(ctypes.byref(crs), h, ptr(wires), ptr(k), ptr(k), *[ptr(x) for x in out]) == ZKT_ERR_SHAPE, (cn, cm)
            assert all((x == np.uint64(PAT)).all() for x in out)
        hq = np.full((n, 4), PAT, np.uint64)
        assert L.zkt_qap_quotient_resident(h, None, ptr(hq)) == ZKT_ERR_SHAPE and L.zkt_qap_quotient_resident(h, ptr(wires), None) == ZKT_ERR_SHAPE
        assert (hq == np.uint64(PAT)).all()
    finally:
        L.zkt_qap_free(h)
