"""Every route through the G1 MSM object, which runs Fq on 13 x 30-bit limbs (fp.h, W = 30) in 14-word memory slots, by linearity against python integers:
the bases are k_i * G, so  sum_i s_i * (k_i * G)  must be  (sum_i k_i s_i mod r) * G, computed here by py_g1_mul.  The bases themselves come from the CPU oracle
(code this object has no part in).  Small sizes on purpose: one bucket piece, the piece merge, the doubling exit and the sum at infinity inside a bucket, the direct
plan with its window join, the batched form, the slot ring and the sharded combine all run at a few hundred terms."""
import ctypes, importlib
import numpy as np
import pytest
from zkt_testlib import oracle, ptr, G1W, R, G1_GEN, g1_arr, g1_from_arr, py_g1_mul, int_to_limbs, limbs_to_int, rand_scalars

pytestmark = pytest.mark.gpu
zk = importlib.import_module("zk-toolkit_amd")
N_MAX = 700
PW = zk.G1_PARTIAL_WORDS


@pytest.fixture(scope="module")
def L():
    zk.init()
    return zk.lib()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


_ref = {}


def _bases():
    """(discrete logs, (N_MAX, 13) host array of k_i * G) — computed once and shared, never modified"""
    if not _ref:
        rng = np.random.Generator(np.random.PCG64(30))
        ks = [int(limbs_to_int(row)) % R or 1 for row in rng.integers(0, 2**64, size=(N_MAX, 4), dtype=np.uint64)]
        _ref["ks"], _ref["pts"] = ks, _points(ks)
    return _ref["ks"], _ref["pts"]


def _points(ks):
    """k * G for every k by the oracle; k = 0 gives the point at infinity"""
    O, n = oracle(), len(ks)
    g = np.zeros((1, G1W), np.uint64); O.zkto_g1_generator(ptr(g))
    karr = np.array([int_to_limbs(k, 4) for k in ks], dtype=np.uint64)
    out = np.zeros((n, G1W), np.uint64)
    assert O.zkto_g1_mul_batch(ptr(np.repeat(g, n, axis=0)), ptr(karr), 4, ptr(out), n, 16) == 0
    return out


def _sc_arr(ss):
    return np.array([int_to_limbs(s, 4) for s in ss], dtype=np.uint64)


def _want(ks, ss):
    return py_g1_mul(G1_GEN, sum(k * s for k, s in zip(ks, ss)) % R)


def _resident(L, pts, ss, partial=None):
    n = len(ss)
    h = ctypes.c_void_p()
    zk.check(L.zkt_g1_bases_upload(ptr(np.ascontiguousarray(pts[:n])), n, ctypes.byref(h)))
    try:
        got = np.zeros((1, G1W), np.uint64)
        zk.check(L.zkt_g1_msm_dev(h, _vp(_to_dev(_sc_arr(ss))), n, None, ptr(got), partial))
        return g1_from_arr(got)[0]
    finally:
        L.zkt_g1_bases_free(h)


def _uniform(seed, n):
    return [int(limbs_to_int(r)) for r in rand_scalars(seed, n)]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 700])
def test_resident_msm_uniform_scalars(L, n):
    ks, pts = _bases()
    ss = _uniform(100 + n, n)
    assert _resident(L, pts, ss) == _want(ks[:n], ss)


def test_all_scalars_equal(L):
    """one hot bucket per window, cut into pieces: k_merge_partials"""
    ks, pts = _bases()
    ss = [0x1234567 * (1 << 200) + 0xABCDEF] * N_MAX
    assert _resident(L, pts, ss) == _want(ks, ss)


def test_scalars_zero_and_r_minus_one_among_the_others(L):
    ks, pts = _bases()
    ss = _uniform(7, N_MAX)
    for i in range(0, N_MAX, 50):
        ss[i] = 0; ss[i + 1] = R - 1
    assert _resident(L, pts, ss) == _want(ks, ss)


@pytest.mark.parametrize("case", ["equal_bases", "opposite_bases", "base_at_infinity"])
def test_special_bases_inside_a_bucket(L, case):
    """equal bases with equal scalars meet in every bucket they enter: P + P, the doubling exit; a base and its negative: the sum at infinity; a base at infinity adds nothing"""
    ks, pts = _bases()
    ks = list(ks)
    ss = _uniform(11, N_MAX)
    if case == "equal_bases":
        ks[1] = ks[0]; ss[1] = ss[0]
    elif case == "opposite_bases":
        ks[1] = R - ks[0]; ss[1] = ss[0]
    else:
        ks[1] = 0
    pts = pts.copy()
    pts[1] = _points([ks[1]])[0]
    assert (g1_from_arr(pts[1:2])[0] is None) == (case == "base_at_infinity")
    assert _resident(L, pts, ss) == _want(ks, ss)


def test_one_shot_host_pointers(L):
    """zkt_g1_msm: the direct plan (every window its own buckets) and k_join_windows"""
    ks, pts = _bases()
    n = 300
    ss = _uniform(300, n)
    got = np.zeros((1, G1W), np.uint64)
    zk.check(L.zkt_g1_msm(ptr(np.ascontiguousarray(pts[:n])), ptr(_sc_arr(ss)), n, ptr(got)))
    assert g1_from_arr(got)[0] == _want(ks[:n], ss)


def test_batched_three_vectors(L):
    ks, pts = _bases()
    n, k = 257, 3
    vs = [_uniform(400 + v, n) for v in range(k)]
    h = ctypes.c_void_p()
    zk.check(L.zkt_g1_bases_upload(ptr(np.ascontiguousarray(pts[:n])), n, ctypes.byref(h)))
    try:
        out = np.zeros((k, G1W), np.uint64)
        zk.check(L.zkt_g1_msm_batch_dev(h, _vp(_to_dev(np.concatenate([_sc_arr(v) for v in vs]))), n, k, n, None, ptr(out), None))
        assert g1_from_arr(out) == [_want(ks[:n], v) for v in vs]
    finally:
        L.zkt_g1_bases_free(h)


def test_submit_collect_ring_of_eight(L):
    ks, pts = _bases()
    n = N_MAX
    vs = [_uniform(500 + s, n) for s in range(8)]
    d = [_to_dev(_sc_arr(v)) for v in vs]
    h = ctypes.c_void_p()
    zk.check(L.zkt_g1_bases_upload(ptr(pts), n, ctypes.byref(h)))
    try:
        for s in range(8):
            zk.check(L.zkt_g1_msm_submit(h, _vp(d[s]), n, None, s))
        for s in range(8):
            got = np.zeros((1, G1W), np.uint64)
            zk.check(L.zkt_g1_msm_collect(h, s, ptr(got), None))
            assert g1_from_arr(got)[0] == _want(ks, vs[s]), s
    finally:
        L.zkt_g1_bases_free(h)


def test_two_shard_partials(L):
    """two halves of 130 terms, each leaving a 42-word Jacobian partial; zkt_g1_jac_sum_dev adds and normalises them.  A coordinate has 13 limbs in a 14-word slot:
    words 13, 27 and 41 of every partial are zero."""
    import torch
    ks, pts = _bases()
    n, half = 130, 65
    ss = _uniform(130, n)
    parts = torch.full((2 * PW,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    for sh in range(2):
        lo = sh * half
        got = _resident(L, pts[lo:lo + half], ss[lo:lo + half], ctypes.c_void_p(parts.data_ptr() + 4 * PW * sh))
        assert got == _want(ks[lo:lo + half], ss[lo:lo + half])
    words = parts.cpu().numpy().view(np.uint32).reshape(2, PW)
    assert (words[:, [13, 27, 41]] == 0).all(), words[:, [13, 27, 41]]
    out = np.zeros((1, G1W), np.uint64)
    zk.check(L.zkt_g1_jac_sum_dev(_vp(parts), 2, None, ptr(out)))
    assert g1_from_arr(out)[0] == _want(ks[:n], ss)
