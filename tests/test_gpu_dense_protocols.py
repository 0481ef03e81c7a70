"""The two dense trusted-setup protocols on the GPU against the exponent model of tests/dense_model.py, at the shapes where their kernels leave the first block and
where the host code slices empty or one-element CRS fields: zkt_groth16_setup / zkt_groth16_prove, zkt_pinocchio_setup / zkt_pinocchio_prove /
zkt_pinocchio_prove_resident on seeded random dense polynomials (setup and prove are linear algebra on the exponents: no satisfiable circuit is needed), and
zkt_pinocchio_verify at the io counts around PIN_FAST_IO on satisfied chain circuits.  Every expected point is generator * (a python integer) through the oracle's
threaded batch multiplication; every comparison is byte equality.  tests/test_dense_model.py proves on the CPU that these cases reach every cell of dense_model.CELLS."""
import ctypes, importlib
import numpy as np
import pytest
import dense_model as D
from zkt_testlib import oracle, ptr, ints_to_arr, limbs_to_int, G1W, G2W, FQ12, R, ZKT_ERR_INV_ZERO, ZKT_ERR_SHAPE
from qap_util import alloc_crs, alloc_pinocchio, alloc_pinocchio_proof, chain_io_circuit, pinocchio_instance

pytestmark = pytest.mark.gpu
zk = importlib.import_module("zk-toolkit_amd")
O = oracle()
arr = lambda xs: ints_to_arr(list(xs), 4)
FILL = 0xAB
size_t = ctypes.c_size_t


@pytest.fixture(scope="module")
def L():
    zk.init()
    return zk.lib()


def assert_points(got, group, scalars, what):
    """the first len(scalars) points of `got` are generator * scalar, byte for byte; whatever the buffer holds beyond them was not written"""
    want = D.expected_points(O, group, scalars)
    k = len(scalars)
    if got[:k].tobytes() != want.tobytes():
        bad = [i for i in range(k) if got[i].tobytes() != want[i].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} of {k} points differ from generator * model scalar, first at index {bad[0]}")
    assert (got[k:] == FILL).all(), f"{what}: written beyond its {k} points"


def filled(bufs):
    for b in bufs.values(): b[:] = FILL
    return bufs


# ---- Groth16 ------------------------------------------------------------------------------------------------------------------------------
def abc():
    return {"A": np.full((1, G1W), FILL, np.uint64), "B": np.full((1, G2W), FILL, np.uint64), "C": np.full((1, G1W), FILL, np.uint64)}


@pytest.mark.parametrize("case", D.g16_cases(), ids=D.case_id)
def test_groth16_setup_and_prove_equal_the_model(L, case):
    rows, n, l = case["shape"]; m = rows - 1
    x = D.groth16_inputs(rows, n, l, 1000 + 7 * rows + n, noncanonical=case["noncanonical"])
    model = D.groth16_crs(x["ui"], x["vi"], x["wi"], n, l, m, *x["trap"])
    U, V, W = arr(x["ui"]), arr(x["vi"]), arr(x["wi"])
    crs, buf = alloc_crs(n, l, m); filled(buf)
    zk.check(L.zkt_groth16_setup(ctypes.byref(crs), ptr(U), ptr(V), ptr(W), *[ptr(arr([t])) for t in x["trap"]]))
    for name, scalars in model.items():
        assert_points(buf[name], D.G16_GROUPS[name], scalars, f"CRS field {name}")
    gt = np.zeros((1, FQ12), np.uint64)
    assert O.zkto_pairing_batch(3, ptr(D.expected_points(O, "g1", model["g1_alpha"])), ptr(D.expected_points(O, "g2", model["g2_beta"])), ptr(gt), 1, 1, None) == 0
    assert buf["gt_alpha_beta"].tobytes() == gt.tobytes(), "CRS field gt_alpha_beta"
    H, rr, ss = arr(x["h"]), arr([x["r"]]), arr([x["s"]])
    runs = [(x["wires"], h_len) for h_len in case["h_lens"]] + ([([0] * rows, n)] if case["zero_wires"] else [])
    for wires, h_len in runs:
        out = abc()
        zk.check(L.zkt_groth16_prove(ctypes.byref(crs), ptr(U), ptr(V), ptr(arr(wires)), ptr(H), h_len, ptr(rr), ptr(ss), *[ptr(out[k]) for k in "ABC"]))
        want = D.groth16_proof(model, x["ui"], x["vi"], wires, x["h"][:h_len], x["r"], x["s"], n, l, m)
        for k in "ABC":
            assert_points(out[k], D.PROOF16_GROUPS[k], [want[k]], f"proof element {k} with h_len {h_len}" + (" and all wires zero" if wires is not x["wires"] else ""))
    out = abc(); H1 = arr(x["h"] + [1])
    assert L.zkt_groth16_prove(ctypes.byref(crs), ptr(U), ptr(V), ptr(arr(x["wires"])), ptr(H1), n + 1, ptr(rr), ptr(ss), *[ptr(out[k]) for k in "ABC"]) == ZKT_ERR_SHAPE   # polynomial.rs:277-279
    assert all((v == FILL).all() for v in out.values())


def test_groth16_setup_refuses_trapdoors_that_are_zero_mod_r(L):
    """values are reduced on load: r and 2r are as much a zero as 0 is (they reach the inversions of gamma and delta, or give a CRS of points at infinity)"""
    rows, n, l = 3, 2, 1
    x = D.groth16_inputs(rows, n, l, 41)
    U, V, W = arr(x["ui"]), arr(x["vi"]), arr(x["wi"])
    for pos in range(5):
        for z in D.ZERO_MOD_R:
            crs, buf = alloc_crs(n, l, rows - 1); filled(buf)
            trap = list(x["trap"]); trap[pos] = z
            assert L.zkt_groth16_setup(ctypes.byref(crs), ptr(U), ptr(V), ptr(W), *[ptr(arr([t])) for t in trap]) == ZKT_ERR_INV_ZERO, (pos, hex(z))
            assert all((b == FILL).all() for b in buf.values()), (pos, hex(z))


# ---- Pinocchio: setup and the two provers -----------------------------------------------------------------------------------------------------
def assert_proof(pb, model, x, h_len, n_io, what):
    want = D.pinocchio_proof(model, x["wires"], x["h"][:h_len], x["delta_v"], x["delta_y"], n_io)
    for name, e in want.items():
        assert_points(pb[name], D.PIN_PROOF_GROUPS[name], [e], f"{what}, h_len {h_len}: proof element {name}")


@pytest.mark.parametrize("case", D.pin_cases(), ids=D.case_id)
def test_pinocchio_setup_and_both_provers_equal_the_model(L, case):
    n_io, n_mid, n, deg = case["shape"]
    x = D.pinocchio_inputs(n_io, n_mid, n, deg, 2000 + 7 * (n_io + n_mid) + deg, noncanonical=case["noncanonical"])
    model = D.pinocchio_crs(x["vi"], x["wi"], x["yi"], n, n_io, n_mid, deg, x["rnd"])
    crs, buf = alloc_pinocchio(n, n_io, n_mid, deg); filled(buf)
    zk.check(L.zkt_pinocchio_setup(ctypes.byref(crs), ptr(arr(x["vi"])), ptr(arr(x["wi"])), ptr(arr(x["yi"])), ptr(arr(x["rnd"]))))
    assert sorted(model) == sorted(buf)
    for name, scalars in model.items():
        assert_points(buf[name], D.PIN_GROUPS[name], scalars, f"CRS field {name}")
    wires, H, dv, dy = arr(x["wires"]), arr(x["h"] + [1]), arr([x["delta_v"]]), arr([x["delta_y"]])
    for h_len in case["h_lens"]:
        pf, pb = alloc_pinocchio_proof(); filled(pb)
        zk.check(L.zkt_pinocchio_prove(ctypes.byref(crs), ptr(wires), ptr(H), h_len, ptr(dv), ptr(dy), ctypes.byref(pf)))
        assert_proof(pb, model, x, h_len, n_io, "one-shot prover")
    pf, pb = alloc_pinocchio_proof(); filled(pb)
    assert L.zkt_pinocchio_prove(ctypes.byref(crs), ptr(wires), ptr(H), deg + 1, ptr(dv), ptr(dy), ctypes.byref(pf)) == ZKT_ERR_SHAPE          # polynomial.rs:289-291
    assert all((v == FILL).all() for v in pb.values())
    pk = ctypes.c_void_p()
    zk.check(L.zkt_pinocchio_pk_create(ctypes.byref(crs), ctypes.byref(pk)))
    try:
        # one handle, every length and then the same lengths downwards: a shorter quotient after a longer one needs the zero padding of the resident buffer
        for h_len in case["resident_h_lens"] + case["resident_h_lens"][::-1]:
            pf, pb = alloc_pinocchio_proof(); filled(pb)
            zk.check(L.zkt_pinocchio_prove_resident(pk, ptr(wires), ptr(H), size_t(h_len), ptr(dv), ptr(dy), ctypes.byref(pf)))
            assert_proof(pb, model, x, h_len, n_io, "resident prover")
        pf, pb = alloc_pinocchio_proof(); filled(pb)
        assert L.zkt_pinocchio_prove_resident(pk, ptr(wires), ptr(H), size_t(deg + 1), ptr(dv), ptr(dy), ctypes.byref(pf)) == ZKT_ERR_SHAPE
        assert all((v == FILL).all() for v in pb.values())
    finally:
        L.zkt_pinocchio_pk_free(pk)


def test_pinocchio_setup_refuses_rnd_values_that_are_zero_mod_r(L):
    n_io, n_mid, n, deg = 1, 2, 2, 2
    x = D.pinocchio_inputs(n_io, n_mid, n, deg, 42)
    V, W, Y = arr(x["vi"]), arr(x["wi"]), arr(x["yi"])
    for pos in range(8):
        for z in D.ZERO_MOD_R:
            crs, buf = alloc_pinocchio(n, n_io, n_mid, deg); filled(buf)
            rnd = list(x["rnd"]); rnd[pos] = z
            assert L.zkt_pinocchio_setup(ctypes.byref(crs), ptr(V), ptr(W), ptr(Y), ptr(arr(rnd))) == ZKT_ERR_INV_ZERO, (pos, hex(z))
            assert all((b == FILL).all() for b in buf.values()), (pos, hex(z))


# ---- Pinocchio: the verifier at the io-count edges ----------------------------------------------------------------------------------------------
class Instance:
    """a key, an honest proof and the statement of chain_io_circuit(n_io): set up and proved on the GPU (both pinned to the model above)"""

    def __init__(self, L, n_io, seed):
        A, B, C, wit = chain_io_circuit(n_io)
        n = len(A)
        V, W, Y, h, max_degree = pinocchio_instance(A, B, C, wit)
        x = D.pinocchio_inputs(n_io, len(wit) - n_io, n, max_degree, seed)
        self.n_io, self.oracle_says = n_io, {}
        self.crs, self.cbuf = alloc_pinocchio(n, n_io, len(wit) - n_io, max_degree)
        zk.check(L.zkt_pinocchio_setup(ctypes.byref(self.crs), ptr(V), ptr(W), ptr(Y), ptr(arr(x["rnd"]))))
        self.pf, self.pbuf = alloc_pinocchio_proof()
        zk.check(L.zkt_pinocchio_prove(ctypes.byref(self.crs), ptr(arr(wit)), ptr(arr(h)), len(h), ptr(arr([x["delta_v"]])), ptr(arr([x["delta_y"]])), ctypes.byref(self.pf)))
        self.io = arr(wit[:n_io] if n_io else [0])             # n_io == 0: one unused row, so that the pointer is a valid one

    def both(self, L, io=None):
        """(the oracle's decision, the library's).  The oracle's is a function of the key, the proof and the statement: each distinct input is evaluated once
        (eleven pairings of most of a second each), the library decides every time."""
        io = self.io if io is None else io
        seen = (io.tobytes(), self.pbuf["h_s"].tobytes())
        if seen not in self.oracle_says: self.oracle_says[seen] = O.zkto_pinocchio_verify(ctypes.byref(self.crs), ctypes.byref(self.pf), ptr(io))
        return self.oracle_says[seen], L.zkt_pinocchio_verify(ctypes.byref(self.crs), ctypes.byref(self.pf), ptr(io))

    def altered(self, i):
        bad = self.io.copy(); bad[i, 0] ^= np.uint64(1)
        return bad

    def both_with_wrong_quotient(self, L):
        """the proof with h_s replaced by the G2 generator: only the divisibility check sees it, whatever the io count"""
        keep = self.pbuf["h_s"].copy()
        self.pbuf["h_s"][:] = self.cbuf["one_g2"]
        try: return self.both(L)
        finally: self.pbuf["h_s"][:] = keep


@pytest.mark.parametrize("n_io", D.VERIFY_IO)
def test_pinocchio_verify_at_the_io_count_edges(L, n_io):
    inst = Instance(L, n_io, 600 + n_io)
    assert inst.both(L) == (1, 1)
    assert inst.both_with_wrong_quotient(L) == (0, 0)
    for i in sorted({0, n_io - 1} & set(range(n_io))):         # the first io wire, and the last: the term a short loop drops
        assert inst.both(L, inst.altered(i)) == (0, 0), f"io wire {i} altered"
        big = inst.io.copy(); big[i] = arr([limbs_to_int(inst.io[i]) + R])[0]
        assert inst.both(L, big) == (1, 1), f"io wire {i} plus r"
    assert inst.both(L) == (1, 1)


def test_pinocchio_verify_over_keys_of_different_sizes(L):
    """D.VERIFY_SEQUENCE: the two-entry table cache holds keys of 12 and 2 io wires, evicts one, finds one again and rebuilds one, with a key without io wires and
    the table-free path (13 io wires) in between; an honest and a bad verification at every step, every decision the oracle's.  The cache is process-wide and not
    empty here (the tests above leave their keys in it), so the first two steps evict those; from then on it holds what dense_model.cache_walk says"""
    keys = {}
    for n_io, key in D.VERIFY_SEQUENCE:
        if key not in keys: keys[key] = Instance(L, n_io, 700 + key)
        assert keys[key].n_io == n_io
    assert len(keys) == 5 and keys[0].cbuf["vk_io"].tobytes() != keys[3].cbuf["vk_io"].tobytes()
    for step, (n_io, key) in enumerate(D.VERIFY_SEQUENCE):
        inst = keys[key]
        assert inst.both(L) == (1, 1), (step, n_io)
        if n_io: assert inst.both(L, inst.altered(n_io - 1)) == (0, 0), (step, n_io)
        else: assert inst.both_with_wrong_quotient(L) == (0, 0), (step, n_io)
