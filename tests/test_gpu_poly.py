"""Dense Fr polynomials on the device (csrc/zkt_poly.hip) against python integers (tests/poly_model.py): products, division with remainder, batch
evaluation, t = prod (x - i), the QAP quotient and the Groth16 prover that computes it.  The shapes come from poly_model's case lists, which follow the
thresholds the source holds; tests/test_poly_model.py proves that they reach every cell of the plan."""
import ctypes, importlib
import numpy as np
import pytest
import poly_model as P
from zkt_testlib import R, ptr, ints_to_arr, arr_to_ints, SplitMix64, G1W, G2W, ZKT_OK, ZKT_ERR_SHAPE
from qap_util import example_cubic, chain_circuit, qap_from_r1cs, dense, alloc_crs

pytestmark = pytest.mark.gpu
zk = importlib.import_module("zk-toolkit_amd")
ZKT_ERR_REMAINDER = 5
MAX_LEN = 1 << 21
NONCANON = [R, R + 1, (1 << 256) - 1]


@pytest.fixture(scope="module")
def L():
    zk.init()
    return zk.lib()


def to_ints(a):
    b = np.ascontiguousarray(a).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def to_arr(xs):
    return np.frombuffer(b"".join(x.to_bytes(32, "little") for x in xs), dtype=np.uint64).reshape(-1, 4).copy() if xs else np.zeros((0, 4), np.uint64)


def rand_arr(seed, n):
    """n canonical elements below 2^254, with r - 1 and 0 among them when there is room"""
    a = np.random.Generator(np.random.PCG64(seed)).integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(2)
    if n >= 4: a[1] = to_arr([R - 1])[0]; a[2] = 0
    return a


def gpu_mul(L, a, b, out=None):
    out = np.zeros((len(a) + len(b) - 1, 4), np.uint64) if out is None else out
    assert L.zkt_fr_poly_mul(ptr(a), len(a), ptr(b), len(b), ptr(out)) == ZKT_OK
    return out


# ---- 1. exact products ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", P.mul_shapes(), ids=lambda s: "%dx%d" % s)
def test_product_equals_the_kronecker_model(L, shape):
    na, nb = shape
    a, b = rand_arr(10 + na, na), rand_arr(20 + nb, nb)
    assert to_ints(gpu_mul(L, a, b)) == P.kron_mul(to_ints(a), to_ints(b))


@pytest.mark.parametrize("shape", [(3, 5), (P.mul_shapes()[4][0], 100), (600, 700)], ids=lambda s: "%dx%d" % s)
def test_zero_operand_and_non_canonical_coefficients(L, shape):
    na, nb = shape
    b = rand_arr(31, nb)
    zero = gpu_mul(L, np.zeros((na, 4), np.uint64), b)
    assert zero.shape == (na + nb - 1, 4) and not zero.any()                    # multiply_by does not normalise
    a = to_ints(rand_arr(32, na)); a[0], a[1], a[-1] = NONCANON
    bb = to_ints(b); bb[0], bb[-1] = NONCANON[2], NONCANON[1]
    assert to_ints(gpu_mul(L, to_arr(a), to_arr(bb))) == P.kron_mul(a, bb)       # reduced on load


@pytest.mark.parametrize("n", [5, 513])
def test_squaring_with_one_pointer(L, n):
    a = rand_arr(40 + n, n)
    out = np.zeros((2 * n - 1, 4), np.uint64)
    assert L.zkt_fr_poly_mul(ptr(a), n, ptr(a), n, ptr(out)) == ZKT_OK
    ai = to_ints(a)
    assert to_ints(out) == P.kron_mul(ai, ai)


def test_product_shape_errors(L):
    a = rand_arr(1, 4); out = np.full((8, 4), 0xAB, np.uint64)
    for args in [(ptr(a), 0, ptr(a), 4, ptr(out)), (ptr(a), 4, ptr(a), 0, ptr(out)), (None, 4, ptr(a), 4, ptr(out)), (ptr(a), 4, None, 4, ptr(out)), (ptr(a), 4, ptr(a), 4, None)]:
        assert L.zkt_fr_poly_mul(*args) == ZKT_ERR_SHAPE
    assert (out == 0xAB).all()
    assert zk.lib().zkt_strerror(ZKT_ERR_REMAINDER).decode() not in ("unknown", "")


# ---- 2. three launches per transform ----------------------------------------------------------------------------------------------
def test_three_launch_transform(L):
    na, nb = P.BIG_MUL
    b = rand_arr(50, nb); bi = to_ints(b)
    terms = [(0, 3), (1, R - 2), (1 << 17, 0x123456789ABCDEF), (1 << 18, R - 1)]
    ai = [0] * na
    for d, c in terms: ai[d] = c
    assert to_ints(gpu_mul(L, to_arr(ai), b)) == P.shifted_sum(terms, bi, na + nb - 1)
    a = rand_arr(51, na)
    out = to_ints(gpu_mul(L, a, b)); ai = to_ints(a)
    rng = SplitMix64(52)
    for _ in range(2):                                                          # a wrong product escapes with probability ~ 2^19 / 2^255
        z = rng.below(R)
        assert P.horner(out, z) == P.horner(ai, z) * P.horner(bi, z) % R


# ---- 3. the length limit -------------------------------------------------------------------------------------------------------
def test_limit_and_one_past_it(L):
    na, nb = P.LIMIT_MUL
    assert na + nb - 1 == MAX_LEN
    b = rand_arr(60, nb + 1)
    a = np.zeros((na + 1, 4), np.uint64); a[0, 0] = 1; a[1 << 20, 0] = 1         # 1 + x^(2^20)
    out = np.full((MAX_LEN + 1, 4), 0xAB, np.uint64)
    assert L.zkt_fr_poly_mul(ptr(a), na + 1, ptr(b), nb, ptr(out)) == ZKT_ERR_SHAPE
    assert L.zkt_fr_poly_mul(ptr(a), na, ptr(b), nb + 1, ptr(out)) == ZKT_ERR_SHAPE
    assert (out == 0xAB).all()
    gpu_mul(L, a[:na], b[:nb], out[:MAX_LEN])
    assert (out[:nb] == b[:nb]).all() and (out[nb:MAX_LEN] == b[:nb]).all()      # b || b, no overlap


# ---- 4. device pointers, a stream of the caller's, the twiddle cache ----------------------------------------------------------------
def test_dev_variant_on_a_side_stream_allocates_nothing_the_second_time(L):
    import torch
    n = 513
    a, b = rand_arr(70, n), rand_arr(71, n)
    want = gpu_mul(L, a, b)
    d_a = torch.from_numpy(a.view(np.int64)).cuda(); d_b = torch.from_numpy(b.view(np.int64)).cuda()
    d_o = torch.zeros((2 * n - 1, 4), dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    assert L.zkt_fr_poly_mul_dev(vp(d_a), n, vp(d_b), n, vp(d_o), ctypes.c_void_p(st.cuda_stream)) == ZKT_OK
    st.synchronize(); torch.cuda.synchronize()
    assert (d_o.cpu().numpy().view(np.uint64) == want).all()
    free1 = torch.cuda.mem_get_info()[0]
    d_o.zero_(); torch.cuda.synchronize()
    assert L.zkt_fr_poly_mul_dev(vp(d_a), n, vp(d_b), n, vp(d_o), ctypes.c_void_p(st.cuda_stream)) == ZKT_OK
    st.synchronize(); torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free1
    assert (d_o.cpu().numpy().view(np.uint64) == want).all()
    assert L.zkt_fr_poly_mul_dev(vp(d_a), 0, vp(d_b), n, vp(d_o), None) == ZKT_ERR_SHAPE


# ---- 5. division ----------------------------------------------------------------------------------------------------------------
def gpu_divrem(L, a, b):
    na, nb = len(a), len(b)
    q = np.full((na - nb + 1, 4), 0xAB, np.uint64); rem = np.full((max(nb - 1, 1), 4), 0xAB, np.uint64); rl = ctypes.c_size_t(1 << 40)
    assert L.zkt_fr_poly_divrem(ptr(a), na, ptr(b), nb, ptr(q), ptr(rem) if nb > 1 else None, ctypes.byref(rl)) == ZKT_OK
    return to_ints(q), to_ints(rem[:nb - 1]), rl.value


def _compose(q, b, rem):
    a = P.kron_mul(q, b)
    return [(x + (rem[i] if i < len(rem) else 0)) % R for i, x in enumerate(a)]


@pytest.mark.parametrize("shape", P.div_shapes(), ids=lambda s: "L%d_nb%d" % s)
def test_divrem_recovers_quotient_and_remainder(L, shape):
    Lq, nb = shape
    q = to_ints(rand_arr(80 + Lq, Lq)); b = to_ints(rand_arr(81 + nb, nb)); rem = to_ints(rand_arr(82, nb - 1))
    b[-1] = 0x1234567 + nb                                                       # non-monic
    if nb > 1 and rem[-1] == 0: rem[-1] = 5
    gq, grem, rl = gpu_divrem(L, to_arr(_compose(q, b, rem)), to_arr(b))
    assert gq == q and grem == rem and rl == nb - 1
    if nb == 2:                                                                  # python synthetic division by (b1 x + b0)
        a = _compose(q, b, rem); inv = pow(b[1], -1, R); sq = [0] * Lq; carry = 0
        for k in range(Lq, 0, -1):
            sq[k - 1] = (a[k] - carry) * inv % R; carry = sq[k - 1] * b[0] % R
        assert gq == sq and grem == [(a[0] - carry) % R]


@pytest.mark.parametrize("shape", [(5, 9), (P.div_shapes()[4][0], 33), (300, 200)], ids=lambda s: "L%d_nb%d" % s)
def test_divrem_exact_short_remainder_zero_leading_and_non_canonical(L, shape):
    Lq, nb = shape
    q = to_ints(rand_arr(90, Lq)); b = to_ints(rand_arr(91, nb)); b[-1] = 77
    gq, grem, rl = gpu_divrem(L, to_arr(_compose(q, b, [])), to_arr(b))          # exact: DivResult::Quotient
    assert gq == q and rl == 0 and grem == [0] * (nb - 1)
    rem = [9, 8, 7] + [0] * (nb - 4)                                             # a remainder with zero high coefficients
    gq, grem, rl = gpu_divrem(L, to_arr(_compose(q, b, rem)), to_arr(b))
    assert gq == q and rl == 3 and grem == rem
    a = _compose(q, b, rem) + [0, 0, 0]                                          # zero leading coefficients of a: q is zero-padded
    gq, grem, rl = gpu_divrem(L, to_arr(a), to_arr(b))
    assert gq == q + [0, 0, 0] and rl == 3 and grem == rem
    b2 = list(b); b2[-1] = R + 77; b2[0] = (b[0] + R) if b[0] + R < (1 << 256) else b[0]      # the same divisor in non-canonical limbs
    a2 = _compose(q, b, rem); a2[0] += R if a2[0] + R < (1 << 256) else 0
    gq, grem, rl = gpu_divrem(L, to_arr(a2), to_arr(b2))
    assert gq == q and rl == 3 and grem == rem


def test_divrem_shape_errors(L):
    a = rand_arr(95, 8); q = np.full((8, 4), 0xAB, np.uint64); rem = np.full((8, 4), 0xAB, np.uint64); rl = ctypes.c_size_t(77)
    for lead in (0, R, None):
        b = to_ints(rand_arr(96, 9 if lead is None else 5))
        if lead is not None: b[-1] = lead
        b = to_arr(b)
        assert L.zkt_fr_poly_divrem(ptr(a), 8, ptr(b), len(b), ptr(q), ptr(rem), ctypes.byref(rl)) == ZKT_ERR_SHAPE       # na < nb for lead None
        assert L.zkt_last_error_index() == len(b) - 1
    assert (q == 0xAB).all() and (rem == 0xAB).all() and rl.value == 77


def test_divrem_large(L):
    Lq, nb = P.BIG_DIV
    b = to_ints(rand_arr(100, nb)); b[-1] = 3
    rem = to_ints(rand_arr(101, nb - 1)); rem[-1] = 11
    terms = [(0, 5), (1, R - 1), (1 << 16, 0xDEADBEEF), (1 << 17, 7)]
    q = [0] * Lq
    for d, c in terms: q[d] = c
    a = P.shifted_sum(terms, b, Lq + nb - 1)
    for i, x in enumerate(rem): a[i] = (a[i] + x) % R
    gq, grem, rl = gpu_divrem(L, to_arr(a), to_arr(b))
    assert gq == q and grem == rem and rl == nb - 1
    a = to_ints(rand_arr(102, Lq + nb - 1))                                      # dense: a(z) == q(z) b(z) + rem(z) at two random points
    gq, grem, rl = gpu_divrem(L, to_arr(a), to_arr(b))
    rng = SplitMix64(103)
    for _ in range(2):
        z = rng.below(R)
        assert P.horner(a, z) == (P.horner(gq, z) * P.horner(b, z) + P.horner(grem, z)) % R
    assert rl == len(P.trim(grem))


def test_divrem_quotient_longer_than_half_the_limit(L):
    """2 L - 1 exceeds ZKT_POLY_MAX_LEN: rev(a) g mod x^L is formed from three products of halves.  Against python synthetic division by b1 x + b0."""
    Lq, nb = P.LONG_QUOTIENT_DIV
    a = to_ints(rand_arr(105, Lq + 1)); b = [0x1234567, 0x89ABCDEF01]
    gq, grem, rl = gpu_divrem(L, to_arr(a), to_arr(b))
    inv = pow(b[1], -1, R); c = b[0] * inv % R; carry = 0; q = [0] * Lq
    for k in range(Lq, 0, -1):
        carry = (a[k] * inv - carry * c) % R; q[k - 1] = carry
    assert gq == q and grem == [(a[0] - q[0] * b[0]) % R] and rl == 1


# ---- 6. t ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", P.t_sizes())
def test_build_t_equals_the_product_tree(L, n):
    out = np.full((n + 2, 4), 0xAB, np.uint64)
    assert L.zkt_qap_build_t(n, ptr(out)) == ZKT_OK
    assert to_ints(out[:n + 1]) == P.tree_t(n) and (out[n + 1] == 0xAB).all()


# ---- 7. evaluation ----------------------------------------------------------------------------------------------------------------
_coeffs = {}


def _eval_coeffs(n):
    if n not in _coeffs:
        a = rand_arr(110, n); _coeffs[n] = (a, to_ints(a))
    return _coeffs[n]


@pytest.mark.parametrize("shape", P.EVAL_SHAPES, ids=lambda s: "n%d_k%d" % s)
def test_eval_batch_equals_horner(L, shape):
    n, k = shape
    a, ai = _eval_coeffs(n)
    rng = SplitMix64(111 + k)
    xs = ([R - 1, 0, 1] + [rng.below(R) for _ in range(k)])[:k]
    out = np.zeros((k, 4), np.uint64)
    assert L.zkt_fr_poly_eval_batch(ptr(a), n, ptr(to_arr(xs)), k, ptr(out)) == ZKT_OK
    assert to_ints(out) == [P.horner(ai, x) for x in xs]


def test_eval_from_1_to_n_and_empty_shapes(L):
    a, ai = _eval_coeffs(1000)
    xs = list(range(1, 41)) + [R + 3]                                             # eval_from_1_to_n is xs = 1..n; a point is reduced on load too
    out = np.zeros((41, 4), np.uint64)
    assert L.zkt_fr_poly_eval_batch(ptr(a), 1000, ptr(to_arr(xs)), 41, ptr(out)) == ZKT_OK
    assert to_ints(out) == [P.horner(ai, x % R) for x in xs]
    assert L.zkt_fr_poly_eval_batch(ptr(a), 1000, None, 0, None) == ZKT_OK
    assert L.zkt_fr_poly_eval_batch(ptr(a), 0, ptr(a), 1, ptr(out)) == ZKT_ERR_SHAPE


# ---- 8. the QAP quotient ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", P.QAP_SIZES)
def test_qap_quotient(L, n):
    rows = 3
    u = [to_ints(rand_arr(120 + i, n)) for i in range(rows)]; v = [to_ints(rand_arr(130 + i, n)) for i in range(rows)]
    w = [None] + [to_ints(rand_arr(140 + i, n)) for i in (1, 2)]
    rng = SplitMix64(150 + n)
    wires = [1, rng.below(R), rng.below(R)]
    comb = lambda M: [sum(wires[i] * M[i][k] for i in range(rows)) % R for k in range(n)]
    ab = P.kron_mul(comb(u), comb(v))
    t = P.tree_t(n)
    hq, rem = (P.long_division(ab, t)) if n > 1 else ([], P.trim(ab))
    rem = rem + [0] * (n - len(rem))
    w[0] = [(rem[k] - wires[1] * w[1][k] - wires[2] * w[2][k]) % R for k in range(n)]      # so that sum wires w = (a b) mod t
    U, V, W, wr = to_arr(sum(u, [])), to_arr(sum(v, [])), to_arr(sum(w, [])), to_arr(wires)
    h = np.full((max(n - 1, 1), 4), 0xAB, np.uint64)
    assert L.zkt_qap_quotient(ptr(U), ptr(V), ptr(W), rows, n, ptr(wr), ptr(h) if n > 1 else None) == ZKT_OK
    if n > 1: assert to_ints(h) == hq and len(hq) == n - 1
    j = n // 2
    w[0][j] = (w[0][j] + 1) % R                                                 # p changes by -x^j: that is the remainder
    W = to_arr(sum(w, [])); h2 = np.full((max(n - 1, 1), 4), 0xAB, np.uint64)
    assert L.zkt_qap_quotient(ptr(U), ptr(V), ptr(W), rows, n, ptr(wr), ptr(h2)) == ZKT_ERR_REMAINDER
    assert L.zkt_last_error_index() == j


# ---- 9. the prover that computes its own quotient ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cubic", "chain16"])
def test_prove_qap_equals_prove_with_python_s_quotient(L, case):
    A, B, C, wit, l = example_cubic() if case == "cubic" else chain_circuit(16)
    n, m = len(A), len(wit) - 1
    ui, vi, wi, h, _ = qap_from_r1cs(A, B, C, wit)
    U, V, W = dense(ui, n), dense(vi, n), dense(wi, n)
    rng = SplitMix64(160 + n)
    fr = lambda x: ints_to_arr([x], 4)
    trap = [fr(rng.below(R - 1) + 1) for _ in range(5)]
    r, s = fr(rng.below(R - 1) + 1), fr(rng.below(R - 1) + 1)
    wires, H = ints_to_arr(wit, 4), ints_to_arr(h, 4)
    crs, bufs = alloc_crs(n, l, m)
    assert L.zkt_groth16_setup(ctypes.byref(crs), ptr(U), ptr(V), ptr(W), *[ptr(t) for t in trap]) == ZKT_OK
    want = (np.zeros((1, G1W), np.uint64), np.zeros((1, G2W), np.uint64), np.zeros((1, G1W), np.uint64))
    assert L.zkt_groth16_prove(ctypes.byref(crs), ptr(U), ptr(V), ptr(wires), ptr(H), len(h), ptr(r), ptr(s), *[ptr(x) for x in want]) == ZKT_OK
    got = (np.full((1, G1W), 0xAB, np.uint64), np.full((1, G2W), 0xAB, np.uint64), np.full((1, G1W), 0xAB, np.uint64))
    assert L.zkt_groth16_prove_qap(ctypes.byref(crs), ptr(U), ptr(V), ptr(W), ptr(wires), ptr(r), ptr(s), *[ptr(x) for x in got]) == ZKT_OK
    for a, b, name in zip(want, got, "ABC"):
        assert a.tobytes() == b.tobytes(), f"proof element {name} differs"
    assert L.zkt_groth16_verify(ctypes.byref(crs), ptr(got[0]), ptr(got[1]), ptr(got[2]), ptr(ints_to_arr(wit[:l + 1], 4)), l + 1) == 1
    bad = list(wit); bad[-1] = (bad[-1] + 1) % R                                 # a wrong witness: t does not divide p
    out = (np.full((1, G1W), 0xAB, np.uint64), np.full((1, G2W), 0xAB, np.uint64), np.full((1, G1W), 0xAB, np.uint64))
    assert L.zkt_groth16_prove_qap(ctypes.byref(crs), ptr(U), ptr(V), ptr(W), ptr(ints_to_arr(bad, 4)), ptr(r), ptr(s), *[ptr(x) for x in out]) == ZKT_ERR_REMAINDER
    assert all((x == 0xAB).all() for x in out)
