"""The G1 bucket accumulation (k_accumulate<G1>, zk-toolkit_amd/csrc/zkt_msm.hip) over the paired mixed addition (curve.h: xyzz_add_aff_paired; fp.h: fp_mul_pair,
fp_sqr_pair, -DZKT_PAIR_MUL) at the starts and exceptional steps of a bucket: one, two and three entries, a doubling and a cancellation at the head and in mid-chain,
every sign pattern, buckets cut into pieces.  Resident MSMs against python integers.

The scalars are small, so the bucket contents are chosen by hand: with fewer than 1024 bases the resident plan cuts 10-bit signed digits, a scalar v <= 512 puts
+P into bucket v - 1 and nothing else, and 1024 - v puts -P there (plus a carry: +2^10 P in bucket 0).  Entries reach a bucket in index order, so the bases
named first are the head of their bucket.  A task is 8 entries at these sizes: longer buckets are cut into pieces whose partial sums are merged (nt != 1).
Bases are k_i * G with small known k_i (R - k for a negated point), so the expected sum is (sum k_i s_i mod r) * G from python integers alone."""
import ctypes, importlib
import numpy as np
import pytest
import msm_plan_model as M
from zkt_testlib import G1W, G1_GEN, Q, R, g1_arr, ptr, py_g1_add, py_g1_mul

pytestmark = pytest.mark.gpu
zk = importlib.import_module("zk-toolkit_amd")
C = 10                                         # msm_plan: c = 10 below 2^10 terms (asserted per case through the plan model)


@pytest.fixture(scope="module")
def L():
    zk.init()
    return zk.lib()


_mult = {}


def _kG(k):
    """k * G for the small k of this file: a running sum, computed once"""
    k %= R
    neg = k > R // 2
    m = R - k if neg else k
    if not _mult:
        acc = None
        for i in range(1, 1200):
            acc = py_g1_add(acc, G1_GEN); _mult[i] = acc
    p = _mult[m]
    return (p[0], -p[1] % Q) if neg else p


def _msm(L, ks, scalars):
    """resident MSM (direct call twice, then submit / collect): the four results, all of which must equal python's"""
    import torch
    n = len(ks)
    assert n < 1024 and M.plan(n, "g1", "resident")["c"] == C
    d_bases = torch.from_numpy(g1_arr([_kG(k) for k in ks]).view(np.int64)).cuda()
    d_s = torch.from_numpy(M.scalars_from_ints(scalars).view(np.int64)).cuda()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    h = ctypes.c_void_p()
    zk.check(L.zkt_g1_bases_from_device(vp(d_bases), n, None, ctypes.byref(h)))
    outs = []
    try:
        for _ in range(2):
            got = np.zeros((1, G1W), np.uint64)
            zk.check(L.zkt_g1_msm_dev(h, vp(d_s), n, None, ptr(got), None)); outs.append(got)
        zk.check(L.zkt_g1_msm_submit(h, vp(d_s), n, None, 0))
        got = np.zeros((1, G1W), np.uint64)
        zk.check(L.zkt_g1_msm_collect(h, 0, ptr(got), None)); outs.append(got)
    finally:
        L.zkt_g1_bases_free(h)
    tot = sum(k * s for k, s in zip(ks, scalars)) % R
    want = g1_arr([py_g1_mul(G1_GEN, tot) if tot else None])
    for i, got in enumerate(outs):
        assert (got == want).all(), f"result {i} (msm_dev, msm_dev again, submit/collect) differs from python integers"
    return M.census(M.scalars_from_ints(scalars), None, n, "g1", "resident")


POS = lambda v: v                              # +P into bucket v - 1
NEG = lambda v: (1 << C) - v                   # -P into bucket v - 1 (and the carry)


@pytest.mark.parametrize("n", [1, 2, 3, 65])
def test_few_terms(L, n):
    """n = 1: a copy; 2: one addition of two affine points; 3: the first addition with ZZ != 1; 65: one bucket of 65 entries in 9 pieces"""
    cen = _msm(L, [3 + i for i in range(n)], [POS(5)] * n)
    assert cen["count"][4] == n


def test_distinct_buckets_of_one_and_two(L):
    """65 terms over buckets of 0, 1 and 2 entries, both signs"""
    ks = [2 + i for i in range(65)]
    sc = [POS(1 + i // 2) if i % 3 else NEG(1 + i // 2) for i in range(65)]
    cen = _msm(L, ks, sc)
    assert set(cen["count"][:40]) >= {1, 2} and 0 in set(cen["count"])


def test_700_terms_over_eight_values(L):
    """buckets of 0, 1, 2, 3 and about 90 entries (eleven or more pieces each), signs mixed"""
    rng = np.random.Generator(np.random.PCG64(3))
    vals = [7, 8, 9, 100, 200, 300, 400, 512]
    sc = [POS(20), POS(21), NEG(21), POS(22), NEG(22), POS(22)]
    for i in range(694):
        v = vals[int(rng.integers(0, 8))]
        sc.append(NEG(v) if v != 512 and rng.integers(0, 2) else POS(v))
    ks = [2 + (i * 7) % 1100 for i in range(700)]
    cen = _msm(L, ks, sc)
    cnt = cen["count"]
    assert cnt[19] == 1 and cnt[20] == 2 and cnt[21] == 3 and cnt[50] == 0 and 60 <= cnt[6] <= 120 and cen["max_nt"] >= 8


@pytest.mark.parametrize("signs", [(0, 0), (0, 1), (1, 0), (1, 1)], ids=["++", "+-", "-+", "--"])
def test_sign_combinations_on_the_first_two_entries(L, signs):
    """a bucket of two and a bucket of four (two more steps of either sign)"""
    f = lambda s, v: NEG(v) if s else POS(v)
    sc = [f(signs[0], 9), f(signs[1], 9), f(signs[0], 33), f(signs[1], 33), f(signs[1], 33), f(signs[0], 33)]
    _msm(L, [11, 12, 13, 14, 15, 16], sc)


def test_same_base_twice_at_the_head_doubles(L):
    _msm(L, [5, 5], [POS(3), POS(3)])
    _msm(L, [5, R - 5, 9], [POS(3), NEG(3), POS(3)])              # +P and -(-P): the doubling through the negated y, then one more
    _msm(L, [5, 5, 9, 10], [NEG(3), NEG(3), POS(3), NEG(3)])


def test_p_and_minus_p_at_the_head_then_more(L):
    """the second entry leaves infinity; the next one restarts the accumulator, the rest take the generic path"""
    _msm(L, [5, R - 5, 9, 10, 11], [POS(3)] * 5)
    _msm(L, [5, 5, 9, 10, 11], [POS(3), NEG(3), NEG(3), POS(3), POS(3)])
    _msm(L, [5, R - 5], [POS(3), POS(3)])                          # the whole sum is infinity


def test_same_base_five_times_in_a_row_doubles_in_mid_chain(L):
    """P, P (2P), P (generic: 3P), ... and with 2P as a base: 2P + 2P with an accumulator that is not affine"""
    _msm(L, [5] * 5, [POS(3)] * 5)
    _msm(L, [5, 5, 10, 20, 40], [POS(3)] * 5)                      # 2P, then + 2P, + 4P, + 8P: every loop step is a doubling
    _msm(L, [5, 5, R - 10, 7], [POS(3), POS(3), POS(3), POS(3)])   # 2P + (-2P): infinity in mid-chain, then a restart
    _msm(L, [5, 5, 10, 7], [NEG(3), NEG(3), NEG(3), POS(3)])       # the same doubling on negated entries


def test_more_than_128_entries_in_one_bucket(L):
    """300 entries in one bucket, signs alternating in blocks: its pieces start at every sign pattern; the partial sums are merged"""
    n = 300
    ks = [2 + i for i in range(n)]
    sc = [NEG(77) if (i // 3) % 2 else POS(77) for i in range(n)]
    cen = _msm(L, ks, sc)
    assert cen["count"][76] == n and cen["max_nt"] > 16
