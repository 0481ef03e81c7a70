"""The status of every host-pointer entry point of csrc/zkt_api.cpp and csrc/zkt_hashsig.cpp for every kind of argument combination, as a literal table: what is
decided before anything is staged (NULL pointers, sizes, n == 0), in which order, and what the error word reports.  One field (fr), one tower degree (fq12), one
group (secp) and the pairings stand for their families: the entry points of a family share their code.  Some of the behaviour is uneven (n == 0 is ZKT_OK in one
call and ZKT_ERR_SHAPE in its neighbour); callers may rely on it, so it is pinned as it is.  n is 0, 1 or 2 throughout.
The NULL-pointer rows of the ECDSA and Ed25519 calls are in test_gpu_ecdsa.py and test_gpu_ed25519.py.

test_arena_regrowth_between_layouts runs tests/stage_regrowth_child.py: the calls of three different slot lists, interleaved, while the arena they share is
reallocated between them."""
import ctypes, importlib, os, subprocess, sys
import numpy as np
import pytest
from zkt_testlib import *

pytestmark = pytest.mark.gpu
zk = importlib.import_module("zk-toolkit_amd")
sz, u64 = ctypes.c_size_t, ctypes.c_uint64


@pytest.fixture(scope="module")
def L():
    zk.init()
    return zk.lib()


def P(a):
    """a numpy array as a pointer argument that needs no declared argtypes"""
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


# ---- inputs (n <= 2) ----
A, B, Z = ints_to_arr([3, 5], 4), ints_to_arr([7, 11], 4), ints_to_arr([1, 0], 4)          # Fr; Z[1] has no inverse
O = np.zeros((2, 4), np.uint64)
E1 = ints_to_arr([5, 6], 1)                                                                 # one-limb exponents
T, TO = np.zeros((2, FQ12), np.uint64), np.zeros((2, FQ12), np.uint64)                      # Fq12 zero: multiplies fine, has no inverse
E32 = np.array([3], np.uint32)
S, SO = secp_arr([SECP_GEN, SECP_GEN]), np.zeros((2, 9), np.uint64)
K = ints_to_arr([2, 3], 4)
U32 = np.zeros(2, np.uint32)
G1, G2, GT = np.zeros((2, G1W), np.uint64), np.zeros((2, G2W), np.uint64), np.zeros((2, FQ12), np.uint64)      # filled by the fixture: (generator, infinity), (generator, generator)
PROG_IN, PROG_OUT, PROG_BAD = np.zeros((1, 24), np.uint64), np.zeros((1, 24), np.uint64), np.zeros(1, np.int32)
OFF5, OFF0, DIG = np.array([5], np.uint64), np.array([0], np.uint64), np.zeros(128, np.uint8)
SKS, KS_BAD, SIGS = ints_to_arr([1, 1], 4), ints_to_arr([1, 0], 4), np.zeros((2, 8), np.uint64)      # nonce 0: the reference would draw another
SHAPE, OK = ZKT_ERR_SHAPE, ZKT_OK

# (call, arguments, status[, element reported by zkt_last_error_index])
TABLE = []
row = lambda *r: TABLE.append(r)
# staged calls: n == 0 is ZKT_OK even with NULL pointers; otherwise NULL a, NULL out, or NULL b of a binary operation is ZKT_ERR_SHAPE
for op in ("add", "sub", "mul"):
    for fam, a, b, o in (("fr", A, B, O), ("fq12", T, T, TO)):
        f = f"zkt_{fam}_{op}_batch"
        row(f, (None, None, None, sz(0)), OK); row(f, (None, P(b), P(o), sz(1)), SHAPE); row(f, (P(a), None, P(o), sz(1)), SHAPE); row(f, (P(a), P(b), None, sz(2)), SHAPE)
        row(f, (P(a), P(b), P(o), sz(1)), OK); row(f, (P(a), P(b), P(o), sz(2)), OK)
for f, a, o in [(f"zkt_fr_{op}_batch", A, O) for op in ("sqr", "neg", "inv", "cube")] + [(f"zkt_fq12_{op}_batch", T, TO) for op in ("neg",)]:
    row(f, (None, None, sz(0)), OK); row(f, (None, P(o), sz(1)), SHAPE); row(f, (P(a), None, sz(2)), SHAPE); row(f, (P(a), P(o), sz(2)), OK)
row("zkt_fr_inv_batch", (P(Z), P(O), sz(1)), OK); row("zkt_fr_inv_batch", (P(Z), P(O), sz(2)), ZKT_ERR_INV_ZERO, 1)
row("zkt_fq12_inv_batch", (None, None, sz(0)), OK); row("zkt_fq12_inv_batch", (None, P(TO), sz(1)), SHAPE); row("zkt_fq12_inv_batch", (P(T), None, sz(1)), SHAPE)
row("zkt_fq12_inv_batch", (P(T), P(TO), sz(2)), ZKT_ERR_INV_ZERO, 0)
row("zkt_debug_dfq12_op", (-1, None, None, None, sz(0)), SHAPE); row("zkt_debug_dfq12_op", (7, P(T), P(T), P(TO), sz(1)), SHAPE)
row("zkt_debug_dfq12_op", (0, None, None, None, sz(0)), OK); row("zkt_debug_dfq12_op", (0, P(T), None, P(TO), sz(1)), SHAPE)
row("zkt_debug_dfq12_op", (0, None, P(T), P(TO), sz(1)), SHAPE); row("zkt_debug_dfq12_op", (1, P(T), P(T), None, sz(1)), SHAPE)
row("zkt_debug_dfq12_op", (0, P(T), P(T), P(TO), sz(2)), OK); row("zkt_debug_dfq12_op", (1, P(T), None, P(TO), sz(2)), OK)
row("zkt_secp_add_batch", (None, None, None, sz(0)), OK); row("zkt_secp_add_batch", (None, P(S), P(SO), sz(1)), SHAPE); row("zkt_secp_add_batch", (P(S), None, P(SO), sz(1)), SHAPE)
row("zkt_secp_add_batch", (P(S), P(S), None, sz(1)), SHAPE); row("zkt_secp_add_batch", (P(S), P(S), P(SO), sz(2)), OK)
for f in ("zkt_secp_is_on_curve_batch", "zkt_secp_in_subgroup_batch"):
    row(f, (None, None, sz(0)), OK); row(f, (None, P(U32), sz(1)), SHAPE); row(f, (P(S), None, sz(1)), SHAPE); row(f, (P(S), P(U32), sz(2)), OK)
for f in ("zkt_tate_batch", "zkt_miller_g1g2_batch", "zkt_weil_batch"):
    row(f, (None, None, None, sz(0)), OK); row(f, (None, P(G2), P(GT), sz(1)), SHAPE); row(f, (P(G1), None, P(GT), sz(1)), SHAPE); row(f, (P(G1), P(G2), None, sz(1)), SHAPE)
    row(f, (P(G1), P(G2), P(GT), sz(1)), OK); row(f, (P(G1), P(G2), P(GT), sz(2)), ZKT_ERR_INFINITY, 1)
row("zkt_miller_g2g1_batch", (None, None, None, sz(0)), OK); row("zkt_miller_g2g1_batch", (None, P(G1), P(GT), sz(1)), SHAPE); row("zkt_miller_g2g1_batch", (P(G2), None, P(GT), sz(1)), SHAPE)
row("zkt_miller_g2g1_batch", (P(G2), P(G1), None, sz(1)), SHAPE); row("zkt_miller_g2g1_batch", (P(G2), P(G1), P(GT), sz(1)), OK); row("zkt_miller_g2g1_batch", (P(G2), P(G1), P(GT), sz(2)), ZKT_ERR_INFINITY, 1)
# group mul and scale: `limbs` outside 1..6 is ZKT_ERR_SHAPE even at n == 0, then n == 0 is ZKT_OK
for f in ("zkt_secp_mul_batch", "zkt_secp_scale_batch"):
    row(f, (P(S), P(K), 0, P(SO), sz(0)), SHAPE); row(f, (P(S), P(K), 7, P(SO), sz(0)), SHAPE); row(f, (P(S), P(K), 7, P(SO), sz(1)), SHAPE)
    row(f, (None, None, 4, None, sz(0)), OK); row(f, (None, P(K), 4, P(SO), sz(1)), SHAPE); row(f, (P(S), None, 4, P(SO), sz(1)), SHAPE); row(f, (P(S), P(K), 4, None, sz(1)), SHAPE)
    row(f, (P(S), P(K), 4, P(SO), sz(1)), OK); row(f, (P(S), P(K), 4, P(SO), sz(2)), OK)
# pow: exp_limbs 0 or > 64 is ZKT_ERR_SHAPE even at n == 0, then n == 0 is ZKT_OK
row("zkt_fr_pow_batch", (P(A), P(E1), sz(0), 0, P(O), sz(0)), SHAPE); row("zkt_fr_pow_batch", (P(A), P(E1), sz(65), 0, P(O), sz(0)), SHAPE); row("zkt_fr_pow_batch", (P(A), P(E1), sz(0), 1, P(O), sz(2)), SHAPE)
row("zkt_fr_pow_batch", (None, None, sz(1), 0, None, sz(0)), OK); row("zkt_fr_pow_batch", (None, P(E1), sz(1), 0, P(O), sz(1)), SHAPE); row("zkt_fr_pow_batch", (P(A), None, sz(1), 0, P(O), sz(1)), SHAPE)
row("zkt_fr_pow_batch", (P(A), P(E1), sz(1), 1, None, sz(1)), SHAPE); row("zkt_fr_pow_batch", (P(A), P(E1), sz(1), 0, P(O), sz(2)), OK); row("zkt_fr_pow_batch", (P(A), P(E1), sz(1), 1, P(O), sz(2)), OK)
for f in ("zkt_fr_pow_seq", "zkt_fr_repeat"):
    row(f, (None, sz(0), None), OK); row(f, (None, sz(1), P(O)), SHAPE); row(f, (P(A), sz(1), None), SHAPE); row(f, (P(A), sz(1), P(O)), OK); row(f, (P(A), sz(2), P(O)), OK)
# the vector forms of a field: n == 0 is ZKT_ERR_SHAPE
row("zkt_fr_sum", (P(A), sz(0), P(O)), SHAPE); row("zkt_fr_sum", (None, sz(1), P(O)), SHAPE); row("zkt_fr_sum", (P(A), sz(1), None), SHAPE); row("zkt_fr_sum", (P(A), sz(1), P(O)), OK); row("zkt_fr_sum", (P(A), sz(2), P(O)), OK)
row("zkt_fr_scale_batch", (P(A), P(B), P(O), sz(0)), SHAPE); row("zkt_fr_scale_batch", (None, P(B), P(O), sz(1)), SHAPE); row("zkt_fr_scale_batch", (P(A), None, P(O), sz(1)), SHAPE)
row("zkt_fr_scale_batch", (P(A), P(B), None, sz(1)), SHAPE); row("zkt_fr_scale_batch", (P(A), P(B), P(O), sz(2)), OK)
# the sum of a group: NULL out first, an empty sum is the point at infinity (test_secp_sum_writes below), n > 0 needs points
row("zkt_secp_sum", (None, sz(0), None), SHAPE); row("zkt_secp_sum", (P(S), sz(1), None), SHAPE); row("zkt_secp_sum", (None, sz(0), P(SO)), OK); row("zkt_secp_sum", (None, sz(1), P(SO)), SHAPE)
row("zkt_secp_sum", (P(S), sz(1), P(SO)), OK); row("zkt_secp_sum", (P(S), sz(2), P(SO)), OK)
# NULL exponent, no limbs or more than 4096 before anything else; then n == 0
row("zkt_fq12_pow_batch", (P(T), None, sz(1), P(TO), sz(0)), SHAPE); row("zkt_fq12_pow_batch", (P(T), P(E32), sz(0), P(TO), sz(0)), SHAPE); row("zkt_fq12_pow_batch", (P(T), P(E32), sz(4097), P(TO), sz(0)), SHAPE)
row("zkt_fq12_pow_batch", (None, P(E32), sz(1), None, sz(0)), OK); row("zkt_fq12_pow_batch", (None, P(E32), sz(1), P(TO), sz(1)), SHAPE); row("zkt_fq12_pow_batch", (P(T), P(E32), sz(1), None, sz(1)), SHAPE)
row("zkt_fq12_pow_batch", (P(T), P(E32), sz(1), P(TO), sz(2)), OK)
# count == 0 before the NULL and steps tests
row("zkt_selftest_fq_program", (u64(7), -1, None, None, None, sz(0)), OK); row("zkt_selftest_fq_program", (u64(7), -1, P(PROG_IN), P(PROG_OUT), P(PROG_BAD), sz(1)), SHAPE)
row("zkt_selftest_fq_program", (u64(7), 4, None, P(PROG_OUT), P(PROG_BAD), sz(1)), SHAPE); row("zkt_selftest_fq_program", (u64(7), 4, P(PROG_IN), None, P(PROG_BAD), sz(1)), SHAPE)
row("zkt_selftest_fq_program", (u64(7), 4, P(PROG_IN), P(PROG_OUT), None, sz(1)), SHAPE); row("zkt_selftest_fq_program", (u64(7), 4, P(PROG_IN), P(PROG_OUT), P(PROG_BAD), sz(1)), OK)
# SHA-256 rejects offsets[n] without messages before its n == 0 test; SHA-512 applies the extent test only, behind n == 0
row("zkt_sha256_batch", (None, P(OFF5), sz(0), P(DIG)), SHAPE); row("zkt_sha256_batch", (None, P(OFF0), sz(0), P(DIG)), OK)
row("zkt_sha512_batch", (None, P(OFF5), sz(0), P(DIG)), OK); row("zkt_sha512_batch", (None, P(OFF0), sz(0), P(DIG)), OK)
# a NULL `retry`: the flags are still read back, and the first flagged element is reported with ZKT_ERR_SHAPE
row("zkt_ecdsa_sign_digest_batch", (P(DIG), P(SKS), P(KS_BAD), sz(1), P(SIGS), None), OK); row("zkt_ecdsa_sign_digest_batch", (P(DIG), P(SKS), P(KS_BAD), sz(2), P(SIGS), None), SHAPE, 1)
row("zkt_ecdsa_sign_batch", (P(DIG), P(np.array([0, 3, 9], np.uint64)), P(SKS), P(KS_BAD), sz(2), P(SIGS), None), SHAPE, 1)
IDS = ["%03d-%s" % (i, r[0][4:]) for i, r in enumerate(TABLE)]


@pytest.fixture(scope="module")
def points(L):
    L.zkt_g1_generator(G1.ctypes.data); G1[1] = 0; G1[1, 12] = 1
    L.zkt_g2_generator(G2.ctypes.data); G2[1] = G2[0]


@pytest.mark.parametrize("r", TABLE, ids=IDS)
def test_status_table(L, points, r):
    name, args, want = r[:3]
    assert getattr(L, name)(*args) == want
    if len(r) > 3:
        assert L.zkt_last_error_index() == r[3]


def test_secp_sum_writes(L):
    out = np.full((1, 9), 0xA5A5A5A5A5A5A5A5, np.uint64)
    assert L.zkt_secp_sum(None, sz(0), P(out)) == ZKT_OK
    assert out.tolist() == [[0] * 8 + [1]]                                # the point at infinity: all zero, flag word 1
    assert L.zkt_secp_sum(P(S), sz(1), P(out)) == ZKT_OK and (out == secp_arr([SECP_GEN])).all()
    assert L.zkt_secp_sum(P(S), sz(2), P(out)) == ZKT_OK and (out == secp_arr([py_secp_add(SECP_GEN, SECP_GEN)])).all()


def test_arena_regrowth_between_layouts():
    child = os.path.join(ROOT, "tests", "stage_regrowth_child.py")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, child], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
