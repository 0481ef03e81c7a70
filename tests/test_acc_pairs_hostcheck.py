"""The paired Fq products (fp.h: fp_mul_pair, fp_sqr_pair) and the mixed addition built on them (curve.h: xyzz_add_aff_paired, the hot loop of k_accumulate<G1>) in the host build of the kernel headers (libzkt_hostcheck.so), against python integers.  No GPU.

The interleaved scans are the device code of one object only (the G1 MSM object, -DZKT_PAIR_MUL); fp_mul_pair_impl / fp_sqr_pair_impl are the same loops with the
pins compiled out, so the column order, the carries and the bounds checked here are the kernel's.  A stand-alone program (tests/c/acc_pairs_check.cpp) runs the same
functions under the address and undefined-behaviour sanitizers."""
import ctypes, os, subprocess
import numpy as np
import pytest
from zkt_testlib import ROOT, Q, R, G1_GEN, SplitMix64, ints_to_arr, arr_to_ints, g1_arr, g1_from_arr, py_g1_add, py_g1_mul

_u32p = ctypes.POINTER(ctypes.c_uint32)
p32 = lambda a: a.ctypes.data_as(_u32p)
EDGE = [0, 1, 2, 3, Q - 1, Q - 2, (Q + 1) // 2, 2**380, (1 << 28) - 1, 1 << 28]       # with the lifts below: 0, p, 2p, 3p and each of them plus a small value


@pytest.fixture(scope="module")
def H():
    so = os.path.join(ROOT, "zk-toolkit_amd", "libzkt_hostcheck.so")
    assert os.path.exists(so), "build first (__graft_entry__.build())"
    return ctypes.CDLL(so)


def _pair(H, op, a, b, c, d, lifts):
    enc = lambda v: ints_to_arr([v], 6)
    o0, o1 = np.zeros((1, 6), np.uint64), np.zeros((1, 6), np.uint64)
    bad = H.zkt_hostcheck_fq_pair(op, p32(enc(a)), p32(enc(b)), p32(enc(c)), p32(enc(d)), lifts, p32(o0), p32(o1))
    assert bad == 0, ("a result left the lazy-limb range", op, a, b, c, d, lifts)
    return arr_to_ints(o0)[0], arr_to_ints(o1)[0]


@pytest.mark.parametrize("op", [0, 1, 2, 3], ids=["mul_pair_impl", "sqr_pair_impl", "mul_pair", "sqr_pair"])
def test_pairs_on_edge_residues_in_every_lazy_form(H, op):
    """every edge value in each operand slot at canonical + {0, 1, 2, 3} p: all 256 lift patterns, the operands rotating through the edge list"""
    k = 0
    for lifts in range(256):
        for rot in range(len(EDGE)):
            a, b, c, d = (EDGE[(rot + 3 * s + k) % len(EDGE)] for s in range(4))
            k += 1
            got = _pair(H, op, a, b, c, d, lifts)
            assert got == ((a * b % Q, c * d % Q) if op in (0, 2) else (a * a % Q, c * c % Q)), (op, a, b, c, d, lifts)


@pytest.mark.parametrize("op", [0, 1], ids=["mul_pair_impl", "sqr_pair_impl"])
def test_pairs_on_random_residues(H, op):
    rng = SplitMix64(2024 + op)
    for _ in range(3000):
        a, b, c, d = (rng.below(Q) for _ in range(4))
        got = _pair(H, op, a, b, c, d, rng.next() & 255)
        assert got == ((a * b % Q, c * d % Q) if op == 0 else (a * a % Q, c * c % Q)), (op, a, b, c, d)


def _neg(p):
    return (p[0], -p[1] % Q)


def _acc(H, mode, p, q, signs, lam=7):
    o = np.zeros((1, 13), np.uint64)
    assert H.zkt_hostcheck_g1_acc(mode, p32(g1_arr([p])), p32(g1_arr([q])), signs, p32(ints_to_arr([lam], 6)), p32(o)) == 0
    return g1_from_arr(o)[0]


@pytest.mark.parametrize("mode", [1, 2], ids=["scaled_accumulator", "from_empty"])
def test_first_steps_of_a_bucket_against_the_affine_group_law(H, mode):
    """generic sums, P + P, P + (-P) and a y = 0 pair, each under all four sign combinations; the accumulator of mode 1 carries ZZ = lambda^2 != 1"""
    rng = SplitMix64(99)
    P, S = py_g1_mul(G1_GEN, 0x1234567), py_g1_mul(G1_GEN, R - 5)
    pts = [(P, S), (S, P), (P, P), (P, _neg(P)), (_neg(S), S), ((5, 0), (5, 0)), ((5, 0), (9, 0))] + \
          [(py_g1_mul(G1_GEN, rng.below(R)), py_g1_mul(G1_GEN, rng.below(R))) for _ in range(6)]
    for p, q in pts:
        for signs in range(4):
            for lam in (1, 7, Q - 3):
                want = py_g1_add(_neg(p) if signs & 1 else p, _neg(q) if signs & 2 else q)
                if p[1] == 0 and q[1] == 0 and p[0] != q[0]:
                    continue                                           # two distinct y = 0 "points": no chord through them lands on this curve; only the equal pair is a case
                assert _acc(H, mode, p, q, signs, lam) == want, (mode, p == q, signs, lam)


def test_under_address_and_undefined_sanitizers(tmp_path):
    """tests/c/acc_pairs_check.cpp (its own main: the functions above on a fixed input list, compared with the unpaired products and with jac_add_aff) built for the host with
    the address and undefined-behaviour sanitizers and run as a program of its own; nothing is loaded into python"""
    exe = tmp_path / "acc_pairs_check"
    subprocess.check_call(["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-option-ignored",
                           "-Wno-unused-value", "-Wno-unused-result", "-I", os.path.join(ROOT, "zk-toolkit_amd", "csrc"), os.path.join(ROOT, "tests", "c", "acc_pairs_check.cpp"), "-o", str(exe)], timeout=900)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "acc_pairs ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
