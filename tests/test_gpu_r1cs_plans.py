"""The Groth16 R1CS prover (csrc/zkt_groth16_r1cs.hip) at every transform size and quotient block plan, against python integers.

Every size is a prefix of ONE asymmetric circuit (qap_util.asym_circuit_sparse: A != B, l = 3, rows of 4096 and 4097 terms, a statement wire and a
witness wire in no constraint).  For each size the proof points A, B, C are the python-integer multiples of the generators given by
qap_util.groth16_proof_scalars, and vk.g1_uvw_stmt the multiples given by qap_util.uvw_stmt_scalars — neither the HIP path nor the oracle on the
checking side.  UNSHARDED reaches every transform size logM = 1 .. 22; SHARDED runs each rank's key in turn on this card and sums the ranks'
Jacobian partials as the exchange step does.  tests/test_r1cs_plan_model.py proves that CASES reach every cell of r1cs_plan_model.CELLS."""
import ctypes, functools, importlib
import numpy as np
import pytest
from zkt_testlib import R, SplitMix64, ints_to_arr, ptr, G1W, G2W, G1_GEN, G2_GEN, g1_arr, g2_arr, g1_from_arr, py_g1_mul, py_g2_mul, to_abi_g2
from qap_util import asym_circuit_sparse, prefix, row_dots, lagrange_at, groth16_proof_scalars, uvw_stmt_scalars, alloc_crs, sparse_struct, LONG_ROWS_AT

pytestmark = pytest.mark.gpu
zk = importlib.import_module("zk-toolkit_amd")

BIG = (1 << 20) + 2
L_STMT, NW0 = 3, 7                 # l, and the wires before v_0: one | 3 statement | 2 witness inputs | 1 unused witness wire
UNSHARDED = [1, 2, 3, 4, 5, 9, 17, 33, 65, 129, 257, 513, 1024, 1025, 1500, 2049, 4097, 5000, 9000, 16385, 20000, 40000, 65537, 100000, 200000,
             262145, 300000, 524290, BIG]
SHARDED = [(5, 5), (1000, 7), (4096, 4), (9000, 16), (20000, 3), (40000, 16), (300000, 6), (524290, 3), (BIG, 8)]
PIPELINED = {5, 1025, 65537, BIG}
ALL_PUBLIC_N = 9


def case(n, nshards=1):
    """the census entry (r1cs_plan_model.census) of a prefix of the shared circuit"""
    long_ = n >= LONG_ROWS_AT + 2
    return dict(n=n, nshards=nshards, l=L_STMT, m=n + NW0 - 1, row_lens=(4096, 4097) if long_ else (), row_max=4097 if long_ else 4,
                col_max=n - 2, unused_stmt=True, unused_wit=True)       # col_max: at least the "one" column of B (every row but the two long ones)


CASES = ([case(n) for n in UNSHARDED] + [case(n, W) for n, W in SHARDED] +
         [dict(n=ALL_PUBLIC_N, l=ALL_PUBLIC_N + NW0 - 2, m=ALL_PUBLIC_N + NW0 - 2)] +
         [dict(reject=k) for k in ("x_in_domain", "n_limit", "nshards>n")])


@pytest.fixture(scope="module")
def L():
    zk.init()
    return zk.lib()


@functools.lru_cache(maxsize=1)
def _base():
    """the shared circuit and its per-constraint values (A w)_j, (B w)_j, (C w)_j, built once"""
    c = asym_circuit_sparse(BIG, seed=2026, l=L_STMT, long_rows=True, unused_stmt=True, unused_wit=True)
    return c, row_dots(*c[:3])


fr = lambda v: ints_to_arr([v], 4)


def _inputs(n):
    rng = SplitMix64(31 * n + 7)
    trap = [fr(rng.below(R - 1) + 1) for _ in range(5)]
    rs = [(fr(rng.below(R - 1) + 1), fr(rng.below(R - 1) + 1)) for _ in range(2)]
    return trap, rs


def _g2_gen_c0c1():
    (x1, x0), (y1, y0) = G2_GEN
    return ((x0, x1), (y0, y1))


def _points(As, Bs, Cs):
    return g1_arr([py_g1_mul(G1_GEN, As)]), g2_arr([to_abi_g2(py_g2_mul(_g2_gen_c0c1(), Bs))]), g1_arr([py_g1_mul(G1_GEN, Cs)])


@functools.lru_cache(maxsize=None)
def _expected(n):
    """(the proof points for both (r, s) pairs, the points of vk.g1_uvw_stmt) of the prefix of n constraints"""
    (circuit, rows) = _base()
    mats, wires, l, m = prefix(circuit, n)
    trap, rs = _inputs(n)
    Lx = lagrange_at(n, int.from_bytes(trap[4].tobytes(), "little"))
    proofs = [_points(*groth16_proof_scalars(mats, wires, l, trap, r, s, Lx=Lx, rows=rows)) for r, s in rs]
    uvw = [None if y == 0 else py_g1_mul(G1_GEN, y) for y in uvw_stmt_scalars(mats, l, trap, Lx=Lx)]
    return proofs, uvw


def _setup(L, mats, n, l, m, trap, shard=0, nshards=1):
    structs = [sparse_struct(*M) for M in mats]
    vk, vbuf = alloc_crs(1, l, m); vk.g1_uvw_wit = None
    pk = ctypes.c_void_p()
    rc = L.zkt_groth16_setup_r1cs_sharded(n, l, m, *[ctypes.addressof(x) for x in structs], *[t.ctypes.data for t in trap], shard, nshards,
                                         ctypes.addressof(vk), ctypes.addressof(pk))
    return rc, vbuf, pk


def _new():
    return np.zeros((1, G1W), np.uint64), np.zeros((1, G2W), np.uint64), np.zeros((1, G1W), np.uint64)


def _same(got, want, what):
    for g, w, name in zip(got, want, "ABC"):
        assert (g == w).all(), f"{what}: proof element {name} differs"


@pytest.mark.parametrize("n", UNSHARDED)
def test_unsharded_proof_and_key_at_every_transform_size(L, n):
    """one key per size: vk.g1_uvw_stmt (with the unused statement wire at infinity) and the proof points; some sizes also through _submit/_collect on both slots"""
    import torch
    mats, wires, l, m = prefix(_base()[0], n)
    trap, rs = _inputs(n)
    proofs, uvw = _expected(n)
    rc, vbuf, pk = _setup(L, mats, n, l, m, trap)
    zk.check(rc)
    try:
        assert g1_from_arr(vbuf["g1_uvw_stmt"]) == uvw, "vk.g1_uvw_stmt"
        got = _new()
        zk.check(L.zkt_groth16_prove_r1cs(pk, wires.ctypes.data, rs[0][0].ctypes.data, rs[0][1].ctypes.data, *[x.ctypes.data for x in got]))
        _same(got, proofs[0], f"n={n}")
        if n in PIPELINED:
            d_w = torch.from_numpy(wires.view(np.int64)).cuda()
            pip = [_new(), _new()]
            for slot in (0, 1):
                zk.check(L.zkt_groth16_prove_r1cs_submit(pk, slot, d_w.data_ptr(), rs[slot][0].ctypes.data, rs[slot][1].ctypes.data))
            for slot in (0, 1):
                zk.check(L.zkt_groth16_prove_r1cs_collect(pk, slot, *[x.ctypes.data for x in pip[slot]]))
                _same(pip[slot], proofs[slot], f"n={n} slot {slot}")
    finally:
        L.zkt_groth16_pk_free(pk)


@pytest.mark.parametrize("n,nshards", SHARDED)
def test_sharded_partials_sum_to_the_python_proof(L, n, nshards):
    """each rank's key in turn, its three Jacobian partials, then zkt_g{1,2}_jac_sum_dev over the ranks: the python-integer proof (not merely the unsharded one)"""
    import torch
    mats, wires, l, m = prefix(_base()[0], n)
    trap, rs = _inputs(n)
    proofs, uvw = _expected(n)
    d_w = torch.from_numpy(wires.view(np.int64)).cuda()
    parts = torch.zeros((nshards, zk.GROTH16_PARTIAL_WORDS), dtype=torch.int32, device="cuda")
    for k in range(nshards):
        rc, vbuf, pk = _setup(L, mats, n, l, m, trap, k, nshards)
        zk.check(rc)
        try:
            assert g1_from_arr(vbuf["g1_uvw_stmt"]) == uvw, f"vk.g1_uvw_stmt of rank {k}"
            zk.check(L.zkt_groth16_prove_r1cs_partials(pk, d_w.data_ptr(), rs[0][0].ctypes.data, rs[0][1].ctypes.data, parts[k].data_ptr()))
        finally:
            L.zkt_groth16_pk_free(pk)
    torch.cuda.synchronize()
    a, b = zk.G1_PARTIAL_WORDS, zk.G1_PARTIAL_WORDS + zk.G2_PARTIAL_WORDS
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    pa, pb, pc = parts[:, :a].contiguous(), parts[:, a:b].contiguous(), parts[:, b:].contiguous()
    got = _new()
    zk.check(L.zkt_g1_jac_sum_dev(vp(pa), nshards, None, ptr(got[0])))
    zk.check(L.zkt_g2_jac_sum_dev(vp(pb), nshards, None, ptr(got[1])))
    zk.check(L.zkt_g1_jac_sum_dev(vp(pc), nshards, None, ptr(got[2])))
    _same(got, proofs[0], f"n={n} over {nshards} ranks")


def test_all_wires_public(L):
    """l = m: no witness wire, an empty uvw_wit part of the C1 set; every wire's uvw point in the verifying key"""
    n = ALL_PUBLIC_N
    mats, wires, l, m = asym_circuit_sparse(n, seed=99, all_public=True)
    trap, rs = _inputs(n)
    rc, vbuf, pk = _setup(L, mats, n, l, m, trap)
    zk.check(rc)
    try:
        want = [None if y == 0 else py_g1_mul(G1_GEN, y) for y in uvw_stmt_scalars(mats, l, trap)]
        assert g1_from_arr(vbuf["g1_uvw_stmt"]) == want
        got = _new()
        zk.check(L.zkt_groth16_prove_r1cs(pk, wires.ctypes.data, rs[0][0].ctypes.data, rs[0][1].ctypes.data, *[x.ctypes.data for x in got]))
        _same(got, _points(*groth16_proof_scalars(mats, wires, l, trap, *rs[0])), "all public")
    finally:
        L.zkt_groth16_pk_free(pk)


def test_x_on_the_domain_is_refused_and_2n_is_not(L):
    """x in {1..2n-1} makes t(x) or one x - j zero: ZKT_ERR_INV_ZERO with the index j - 1 = x - 1 of the zero; x = 2n is the first point off it and proves"""
    n = 17
    mats, wires, l, m = asym_circuit_sparse(n, seed=17, l=2)
    trap, rs = _inputs(n)
    for x in (1, n, n + 1, 2 * n - 1):
        rc, _, pk = _setup(L, mats, n, l, m, trap[:4] + [fr(x)])
        assert rc == zk.ZKT_ERR_INV_ZERO and not pk.value, x
        assert L.zkt_last_error_index() == x - 1, x
    trap = trap[:4] + [fr(2 * n)]
    rc, vbuf, pk = _setup(L, mats, n, l, m, trap)
    zk.check(rc)
    try:
        got = _new()
        zk.check(L.zkt_groth16_prove_r1cs(pk, wires.ctypes.data, rs[0][0].ctypes.data, rs[0][1].ctypes.data, *[x.ctypes.data for x in got]))
        _same(got, _points(*groth16_proof_scalars(mats, wires, l, trap, *rs[0])), "x = 2n")
        assert g1_from_arr(vbuf["g1_uvw_stmt"]) == [None if y == 0 else py_g1_mul(G1_GEN, y) for y in uvw_stmt_scalars(mats, l, trap)]
    finally:
        L.zkt_groth16_pk_free(pk)


def test_sizes_past_the_limit_are_refused_up_front(L):
    """n = ZKT_R1CS_MAX_N + 1 = 2^21 (empty rows) and more ranks than constraints: ZKT_ERR_SHAPE, no key; the library proves correctly afterwards"""
    from r1cs_plan_model import MAX_N
    n = MAX_N + 1
    rp = np.zeros(n + 1, np.uint64); col = np.zeros(1, np.uint32); val = np.zeros((1, 4), np.uint64)
    trap, rs = _inputs(5)
    rc, _, pk = _setup(L, [(rp, col, val)] * 3, n, 1, 1, trap)
    assert rc == zk.ZKT_ERR_SHAPE and not pk.value
    mats, wires, l, m = prefix(_base()[0], 3)
    for shard in (0, 3):
        rc, _, pk = _setup(L, mats, 3, l, m, trap, shard, 4)
        assert rc == zk.ZKT_ERR_SHAPE and not pk.value
    mats, wires, l, m = prefix(_base()[0], 5)
    trap, rs = _inputs(5)
    rc, _, pk = _setup(L, mats, 5, l, m, trap)
    zk.check(rc)
    try:
        got = _new()
        zk.check(L.zkt_groth16_prove_r1cs(pk, wires.ctypes.data, rs[0][0].ctypes.data, rs[0][1].ctypes.data, *[x.ctypes.data for x in got]))
        _same(got, _expected(5)[0][0], "after the refusals")
    finally:
        L.zkt_groth16_pk_free(pk)
